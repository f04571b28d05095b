"""Linear probing on the MI355X: the probe's kernels of csrc/classify.hip against torch in float64 on the CPU, the ViT trunk + pooling against
the CPU oracle's pieces, LARS against the reference's own optimizer (tests/golden/lars.npz), and three probe steps end to end.

Bars: the fp32 kernels are held to the elementwise bars the fp32 loss kernels have in tests/test_ops_gpu.py (values rtol 2e-5 / atol 1e-6,
gradients rtol 1e-4 / atol 1e-7: fp32 round-off of a length-D or length-K reduction); trunk features to the latent bar of
test_standalone_encoder_decoder_loss_match_oracle (atol 2e-4, rtol 1e-4) in fp32 and to test_micro_bf16_mfma_path_tracks_fp32's bar for
tensors (cosine > 0.98) in bf16; losses to LOSS_RTOL."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from finetune_ref import G, GRAD, LOSS_RTOL, ROOT, VAL, VIT_MICRO, _ce_case, assert_close, guarded, guards_intact, micro_sd, oracle_features, rnd, write_pretrain_checkpoint

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


# ------------------------------------------------------------------------------------------------ pooling + final norm
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("D", [128, 768, 1280])
@pytest.mark.parametrize("T", [2, 17, 197])
def test_probe_pool_vs_torch(ops, T, D, N, dtype):
    x = rnd(N, T, D, seed=T + D + N).to(dtype)
    gamma, beta = 1 + 0.1 * rnd(D, seed=1), 0.1 * rnd(D, seed=2)
    xd = x.double()
    for gp in (True, False):
        ref = F.layer_norm(xd[:, 1:].mean(1) if gp else xd[:, 0], (D,), gamma.double(), beta.double(), 1e-6)
        big, feat = guarded(N, D)
        ops.probe_pool_fwd(x.cuda(), gamma.cuda(), beta.cuda(), feat, gp)
        assert_close(feat, ref, *VAL, f"pool gp={gp} T={T} D={D} N={N} {dtype}")
        assert guards_intact(big)


def test_probe_pool_refuses_a_mean_over_nothing(ops):
    import csmae_hip
    x, w = torch.zeros(2, 1, 128, device="cuda"), torch.ones(128, device="cuda")
    feat = torch.zeros(2, 128, device="cuda")
    with pytest.raises(csmae_hip.CsmaeError, match="nothing to average"):
        ops.probe_pool_fwd(x, w, w, feat, True)
    ops.probe_pool_fwd(x, w, w, feat, False)   # the cls token alone is fine


# ------------------------------------------------------------------------------------------------ BatchNorm1d over the batch
@pytest.mark.parametrize("N", [2, 5, 128])
@pytest.mark.parametrize("D", [128, 768])
def test_bn1d_two_training_calls_then_eval(ops, N, D):
    bn = torch.nn.BatchNorm1d(D, affine=False, eps=1e-6).double()
    rm, rv = torch.zeros(D, device="cuda"), torch.ones(D, device="cuda")
    nbt = torch.zeros((), dtype=torch.int64, device="cuda")
    for call, training in enumerate((True, True, False)):
        x = rnd(N, D, seed=10 * N + call, scale=1.5) + 0.3
        bn.train(training)
        ref = bn(x.double())
        big, y = guarded(N, D)
        ops.bn1d_fwd(x.cuda(), y, rm, rv, nbt, eps=1e-6, momentum=0.1, training=training)
        assert_close(y, ref, *VAL, f"bn N={N} D={D} call {call}")
        assert_close(rm, bn.running_mean, *VAL, "running_mean")
        assert_close(rv, bn.running_var, *VAL, "running_var")
        assert guards_intact(big)
    assert int(nbt) == int(bn.num_batches_tracked) == 2


def test_bn1d_refuses_one_sample_in_training_before_any_launch(ops):
    x = torch.zeros(1, 128)   # a CPU tensor: the refusal comes before the pointer check, let alone a launch
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ops.bn1d_fwd(x, x.clone(), torch.zeros(128), torch.ones(128), training=True)
    xg, rm, rv = torch.ones(1, 128, device="cuda"), torch.full((128,), 0.5, device="cuda"), torch.full((128,), 4.0, device="cuda")
    y = torch.empty(1, 128, device="cuda")
    ops.bn1d_fwd(xg, y, rm, rv, training=False)
    assert_close(y, torch.full((1, 128), 0.25), *VAL, "eval with one sample")


# ------------------------------------------------------------------------------------------------ classifier + cross-entropy
@pytest.mark.parametrize("N", [1, 3, 128])
@pytest.mark.parametrize("K", [2, 5, 62, 1000])
def test_head_linear_and_softmax_ce_vs_torch_fp64(ops, K, N):
    D = 200
    x, w, b = rnd(N, D, seed=N + K), rnd(K, D, seed=N + K + 1, scale=0.1), rnd(K, seed=N + K + 2, scale=0.1)
    big, out = guarded(N, K)
    ops.head_linear_fwd(x.cuda(), w.cuda(), b.cuda(), out)
    assert_close(out, F.linear(x.double(), w.double(), b.double()), *VAL, f"linear fwd N={N} K={K}")
    assert guards_intact(big)
    # cross-entropy, its gradient and the hit counts
    logits, labels = _ce_case(N, K, seed=7 * N + K)
    lr = logits.double().requires_grad_(True)
    ref = F.cross_entropy(lr, labels)
    gout = 0.7
    (ref * gout).backward()
    loss = torch.full((1,), float("nan"), device="cuda")
    counts = torch.tensor([3.0, 4.0], device="cuda")
    bigd, dl = guarded(N, K)
    ops.softmax_ce(logits.cuda(), labels.cuda(), loss, dlogits=dl, counts=counts, gout=torch.tensor([gout], device="cuda"))
    assert_close(loss[0], ref, *VAL, f"ce N={N} K={K}")
    assert_close(dl, lr.grad, *GRAD, "dlogits")
    assert guards_intact(bigd)
    hits = [int((logits.topk(min(k, K), dim=1).indices == labels[:, None]).any(1).sum()) for k in (1, 5)]
    assert counts.tolist() == [float(hits[0]), float(hits[1])], (counts.tolist(), hits)
    ops.softmax_ce(logits.cuda(), labels.cuda(), loss, counts=counts, accumulate_counts=True)   # no gradient asked for, counts accumulate
    assert counts.tolist() == [2.0 * hits[0], 2.0 * hits[1]]
    # classifier backward from that gradient: written, then accumulated with an upstream scale
    xr, wr, br = x.double(), w.double().requires_grad_(True), b.double().requires_grad_(True)
    d = lr.grad
    (F.linear(xr, wr, br) * d).sum().backward()
    bigw, dw = guarded(K, D)
    db = torch.full((K,), float("nan"), device="cuda")
    dlg = d.float().cuda()
    ops.head_linear_bwd(dlg, x.cuda(), dw, db)
    assert_close(dw, wr.grad, *GRAD, "dW")
    assert_close(db, br.grad, *GRAD, "db")
    ops.head_linear_bwd(dlg, x.cuda(), dw, db, accumulate=True, gscale=torch.tensor([0.5], device="cuda"))
    assert_close(dw, 1.5 * wr.grad, *GRAD, "dW accumulated")
    assert_close(db, 1.5 * br.grad, *GRAD, "db accumulated")
    assert guards_intact(bigw)


def test_softmax_ce_out_of_range_label_indexes_nothing(ops):
    N, K = 4, 5
    logits, labels = _ce_case(N, K, seed=3)
    for bad in (K, -1, 2 ** 40):
        lab = labels.clone()
        lab[2] = bad
        loss, counts = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda")
        big, dl = guarded(N, K)
        ops.softmax_ce(logits.cuda(), lab.cuda(), loss, dlogits=dl, counts=counts)
        assert bool(torch.isnan(loss[0])) and guards_intact(big)
        keep = [0, 1, 3]
        hits = [int((logits[keep].topk(k, dim=1).indices == labels[keep][:, None]).any(1).sum()) for k in (1, 5)]
        assert counts.tolist() == [float(hits[0]), float(hits[1])]
        lr = logits.double().requires_grad_(True)
        F.cross_entropy(lr[keep], labels[keep], reduction="sum").div(N).backward()
        assert_close(dl[keep], lr.grad[keep], *GRAD, "rows with a valid label")
        assert bool(torch.isnan(dl[2]).all())


# ------------------------------------------------------------------------------------------------ LARS
def test_lars_matches_the_reference_after_every_step(ops):
    """util.lars.LARS (the HIP kernel) on the inputs of tests/lars_cases.py against the reference's float64 run.  The float64 run starts
    from the same float32 numbers, so the difference is the kernel's fp32 round-off: a handful of roundings per element (<= 3e-7 relative)
    plus the relative error of q from two blocked fp32 sums of squares (<= 1e-6), per step: mu within 1e-5, p — which moves by lr * mu,
    a small fraction of itself — within 1e-6, both with an absolute floor of 1e-7 of the tensor's largest entry."""
    import lars_cases as C
    from util.lars import LARS
    gold = np.load(os.path.join(G, "lars.npz"))
    stat = lambda t: np.array([t.double().norm().item(), t.double().sum().item()])
    for name, (shapes, wd, _, _) in C.CASES.items():
        params, grads = C.inputs(name)
        for i, p in enumerate(params):
            np.testing.assert_allclose(stat(p), gold[f"{name}_in_p{i}"], rtol=1e-9, atol=1e-12, err_msg="inputs differ from the golden run's")
        ps = [torch.nn.Parameter(p.cuda()) for p in params]
        opt = LARS(ps, lr=C.LR, weight_decay=wd, momentum=C.MOMENTUM, trust_coefficient=C.TRUST)
        for step in range(C.STEPS):
            for i, (p, g) in enumerate(zip(ps, grads[step])):
                np.testing.assert_allclose(stat(g), gold[f"{name}_in_g{step}_{i}"], rtol=1e-9, atol=1e-12)
                p.grad = g.cuda()
            opt.step()
            for i, p in enumerate(ps):
                idx = C.sample_index(p.numel())
                for what, t, rtol in (("p", p.detach(), 1e-6), ("mu", opt.state[p]["mu"], 1e-5)):
                    ref = torch.from_numpy(gold[f"{name}_s{step}_{what}{i}"])
                    full = gold[f"{name}_s{step}_{what}stat{i}"]
                    assert_close(t.reshape(-1).cpu()[idx], ref, rtol, 1e-7 * float(ref.abs().max()), f"lars {name} step {step} {what}{i}")
                    got = stat(t.cpu())
                    assert abs(got[0] - full[0]) <= 1e-5 * full[0] + 1e-30, (name, step, what, got, full)
                    assert abs(got[1] - full[1]) <= 1e-5 * full[0] * np.sqrt(t.numel()) + 1e-30, (name, step, what, got, full)
        assert set(opt.state_dict()["state"][0]) == {"mu"}


# ------------------------------------------------------------------------------------------------ trunk + pooling, end to end
@pytest.fixture(scope="module")
def trunk():
    """Micro weights under timm's names, the images, and the oracle's features for both pooling modes (computed once)."""
    from util.checkpoint_keys import to_vit_keys
    sd = {k: v.float() for k, v in to_vit_keys(micro_sd()).items()}
    imgs = rnd(3, 3, 64, 64, seed=5)
    fc = (1 + 0.1 * rnd(128, seed=6), 0.1 * rnd(128, seed=7))
    sd["norm.weight"], sd["norm.bias"] = 1 + 0.1 * rnd(128, seed=8), 0.1 * rnd(128, seed=9)   # (the pre-training model leaves encoder_norm at its init)
    feats = {True: oracle_features(sd, imgs, True, *fc), False: oracle_features(sd, imgs, False, sd["norm.weight"], sd["norm.bias"])}
    return sd, imgs, fc, feats


def build_vit(sd, global_pool, fc, num_classes=5):
    import models_vit
    vit = models_vit.vit_base_patch16(num_classes=num_classes, global_pool=global_pool, **VIT_MICRO)
    msg = vit.load_state_dict(sd, strict=False)
    assert set(msg.missing_keys) == {"head.weight", "head.bias"} | ({"fc_norm.weight", "fc_norm.bias"} if global_pool else set())
    if global_pool:
        vit.fc_norm.weight.data.copy_(fc[0])
        vit.fc_norm.bias.data.copy_(fc[1])
    return vit.probe_mode().cuda()


@pytest.mark.parametrize("global_pool", [True, False])
def test_trunk_and_pool_match_the_oracle(ops, trunk, global_pool):
    sd, imgs, fc, feats = trunk
    vit = build_vit(sd, global_pool, fc)
    vit.compute_dtype = torch.float32
    f32 = vit.forward_features(imgs.cuda()).cpu()
    ref = feats[global_pool]
    print("fp32 max|err|", float((f32 - ref).abs().max()))
    assert torch.allclose(f32, ref, atol=2e-4, rtol=1e-4), float((f32 - ref).abs().max())
    vit.compute_dtype = torch.bfloat16
    b16 = vit.forward_features(imgs.cuda()).cpu()
    cos = F.cosine_similarity(b16, ref, dim=1)
    print("bf16 cosine", cos.tolist())
    assert bool((cos > 0.98).all()), cos.tolist()
    vit.compute_dtype = None   # autocast selects the bf16 engine, as for the pre-training models
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(vit.forward_features(imgs.cuda()).cpu(), b16)
    assert torch.equal(vit.forward_features(imgs.cuda()).cpu(), f32)
    logits = vit(imgs.cuda())
    assert logits.shape == (3, 5) and bool(torch.isfinite(logits).all())


def lars_rule(params, mus, lr, wd, momentum=0.9, trust=0.001):
    """util/lars.py's update, restated: matrices get weight decay and the trust ratio, vectors neither."""
    for p, mu in zip(params, mus):
        dp = p.grad
        if p.ndim > 1:
            dp = dp + wd * p
            pn, un = p.norm(), dp.norm()
            dp = dp * (trust * pn / un if pn > 0 and un > 0 else 1.0)
        mu.mul_(momentum).add_(dp)
        p.sub_(lr * mu)


@pytest.fixture(scope="module")
def pretrain_checkpoint(tmp_path_factory):
    return write_pretrain_checkpoint(tmp_path_factory.mktemp("pretrain"))


@pytest.mark.parametrize("global_pool", [True, False])
def test_three_probe_steps_match_torch(ops, pretrain_checkpoint, global_pool):
    import main_linprobe
    import models_vit
    from util.checkpoint_keys import to_vit_keys
    from util.lars import LARS
    N, K, lr, wd = 4, 5, 0.1, 0.1
    torch.manual_seed(3)
    vit = models_vit.vit_base_patch16(num_classes=K, global_pool=global_pool, **VIT_MICRO)
    msg = main_linprobe.load_pretrained(vit, pretrain_checkpoint, transform_keys=True)
    assert set(msg.missing_keys) == {"head.weight", "head.bias"} | ({"fc_norm.weight", "fc_norm.bias"} if global_pool else set())
    vit.probe_mode()
    imgs, labels = rnd(N, 3, 64, 64, seed=11), torch.tensor([0, 3, 3, 1])
    # ---- the same three steps on the CPU with torch
    sd = {k: v.float() for k, v in to_vit_keys(micro_sd()).items()}
    norm = vit.fc_norm if global_pool else vit.norm
    feats = oracle_features(sd, imgs, global_pool, norm.weight.detach().clone(), norm.bias.detach().clone())
    bn, lin = torch.nn.BatchNorm1d(128, affine=False, eps=1e-6), torch.nn.Linear(128, K)
    lin.load_state_dict({k: v.clone() for k, v in vit.head[1].state_dict().items()})
    mus, want = [torch.zeros_like(p) for p in lin.parameters()], []
    for _ in range(3):
        loss = F.cross_entropy(lin(bn(feats)), labels)
        lin.zero_grad()
        loss.backward()
        with torch.no_grad():
            lars_rule(list(lin.parameters()), mus, lr, wd)
        want.append(float(loss))
    # ---- on the chip
    vit.cuda().train()
    vit.compute_dtype = torch.float32
    frozen = {n: p.detach().clone() for n, p in vit.named_parameters() if not n.startswith("head.")}
    opt = LARS(vit.head.parameters(), lr=lr, weight_decay=wd)
    got = []
    for _ in range(3):
        loss, logits = vit(imgs.cuda(), labels.cuda())
        assert loss.requires_grad and not logits.requires_grad
        loss.backward()
        opt.step()
        opt.zero_grad(set_to_none=False)
        got.append(float(loss))
    print("loss", got, want)
    for a, b in zip(got, want):
        assert abs(a - b) <= LOSS_RTOL * abs(b), (got, want)
    for (n, p), q in zip(vit.head[1].named_parameters(), lin.parameters()):
        scale = float(q.abs().max())
        print(n, "max|err|", float((p.detach().cpu() - q.detach()).abs().max()), "scale", scale)
        np.testing.assert_allclose(p.detach().cpu().numpy(), q.detach().numpy(), rtol=2e-3, atol=2e-4 * scale + 1e-9, err_msg=n)   # the gradient bar of test_micro_variants_fp32_vs_reference_and_oracle
    assert torch.allclose(vit.head[0].running_mean.cpu(), bn.running_mean, atol=2e-4, rtol=1e-4)   # the latent bar: the statistics are means of features
    assert torch.allclose(vit.head[0].running_var.cpu(), bn.running_var, atol=2e-4, rtol=1e-3)
    assert int(vit.head[0].num_batches_tracked) == 3
    for n, p in vit.named_parameters():
        if not n.startswith("head."):
            assert torch.equal(p.detach(), frozen[n]) and p.grad is None, n
    # ---- evaluate on the same batch against torch in eval mode
    stats = main_linprobe.evaluate([(imgs.cuda(), labels.cuda())], vit, "cuda")
    with torch.no_grad():
        ref_logits = lin(bn.eval()(feats))
    acc = [100.0 * float((ref_logits.topk(min(k, K), dim=1).indices == labels[:, None]).any(1).float().mean()) for k in (1, 5)]
    assert stats["acc1"] == acc[0] and stats["acc5"] == acc[1] == 100.0, (stats, acc)
    assert abs(stats["loss"] - float(F.cross_entropy(ref_logits, labels))) <= LOSS_RTOL * stats["loss"]


def test_cli_synthetic_epoch_writes_a_checkpoint_that_resume_restores(ops, pretrain_checkpoint, tmp_path):
    import main_linprobe
    import models_vit
    import util.misc as misc
    from util.lars import LARS
    flags = ["--dataset_type", "synthetic", "--epochs", "1", "--model", "vit_base_patch16", "--embed_dim", "128", "--depth", "2", "--num_heads", "2",
             "--input_size", "64", "--batch_size", "4", "--nb_classes", "5", "--synthetic_len", "3", "--global_pool", "--weight_decay", "0.1",
             "--output_dir", str(tmp_path), "--device", "cuda"]
    run = subprocess.run([sys.executable, "main_linprobe.py", "--finetune", pretrain_checkpoint, "--transform_checkpoint_keys"] + flags,
                         cwd=os.path.join(ROOT, "cross-scale-mae_amd"), capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    path = tmp_path / "checkpoint-0.pth"
    assert path.exists() and (tmp_path / "log.jsonl").exists()
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert float(ckpt["model"]["head.0.num_batches_tracked"]) == 3 and float(ckpt["model"]["head.1.weight"].abs().max()) > 0
    # what --resume does (main_linprobe.main up to the epoch loop): model + probe head, LARS, misc.load_model
    args = main_linprobe.get_args_parser().parse_args(flags + ["--resume", str(path)])
    vit = models_vit.vit_base_patch16(num_classes=5, global_pool=True, **VIT_MICRO).probe_mode().cuda()
    opt = LARS(vit.head.parameters(), lr=0.1, weight_decay=0.1)
    misc.load_model(args=args, model_without_ddp=vit, optimizer=opt, loss_scaler=None)
    assert args.start_epoch == 1
    own = vit.state_dict()
    for k, v in ckpt["model"].items():
        assert torch.equal(own[k].cpu(), v), k
    state = ckpt["optimizer"]["state"]
    assert len(state) == 2
    for i, p in enumerate(vit.head.parameters()):
        assert torch.equal(opt.state[p]["mu"].cpu(), state[i]["mu"]) and opt.state[p]["mu"].is_cuda and float(state[i]["mu"].abs().max()) > 0
