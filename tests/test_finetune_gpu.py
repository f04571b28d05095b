"""End-to-end fine-tuning on the MI355X: the fine-tune kernels of csrc/classify.hip against torch in float64 on the CPU (outputs in NaN-guarded
buffers), three fine-tune steps of the micro ViT against the CPU restatement stepped with torch.optim.AdamW, gradient accumulation,
reproducibility, and the command line.

Bars: VAL / GRAD of finetune_ref.py for the fp32 kernels (fp32 round-off of a length-D / length-K reduction; the absolute floor of GRAD,
1e-7, is meant for gradients of a mean loss — the upstream gradients fed to the kernels here are of that size, 0.1 and below).  A bf16 output
is one bf16 rounding away from the fp32 result: |bf16(v) - ref| <= 2^-8 |v| + |v - ref| (half an ulp of 8 significant bits), so its bound is
2^-8 |ref| on top of GRAD.  The
end-to-end bars are the ones the issue names: rtol 2e-3 / atol 2e-4 x scale of test_micro_variants_fp32_vs_reference_and_oracle for fp32
gradients and parameters, LOSS_RTOL for fp32 losses; cosine >= 0.98 per tensor and the bf16 loss bar of
test_full_size_vitb_224_n128_vs_reference for the bf16 engine."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import finetune_ref as R
from finetune_ref import GRAD, LOSS_RTOL, VAL, VIT_MICRO, _ce_case, assert_close, guarded, guards_intact, rnd, write_pretrain_checkpoint

pytestmark = pytest.mark.gpu
ROOT = R.ROOT
BF16_EPS = 2.0 ** -8   # one round-to-nearest bf16 rounding: half an ulp of 8 significant bits, relative to the bottom of its binade


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


# ------------------------------------------------------------------------------------------------ pooling + final norm, backward
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("D", [128, 768, 1280])
@pytest.mark.parametrize("T", [2, 17, 197])
def test_probe_pool_bwd_vs_torch_autograd_fp64(ops, T, D, N, dtype):
    # tokens of a sample share a row (what pooling extracts) under 0.3 x noise: the pooled row keeps a spread of ~1, so LayerNorm's rstd is ~1.  (With
    # iid N(0, 1) tokens the mean over 196 of them has a spread of 0.07 and rstd = 14 multiplies every fp32 round-off of the pooled sum: 3e-7 absolute
    # on a dgamma element that cancels to 2e-3, measured — round-off of the forward's sum, three times GRAD's absolute floor.)
    x = (rnd(N, 1, D, seed=T + D + N) + 0.3 * rnd(N, T, D, seed=T + D + N + 1)).to(dtype)
    gamma, beta = 1 + 0.1 * rnd(D, seed=1), 0.1 * rnd(D, seed=2)
    dfeat = rnd(N, D, seed=3, scale=0.1)
    rt, at = GRAD if dtype == torch.float32 else (GRAD[0] + BF16_EPS, GRAD[1])
    for gp in (True, False):
        xd, gd, bd = x.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        feat = F.layer_norm(xd[:, 1:].mean(1) if gp else xd[:, 0], (D,), gd, bd, 1e-6)
        (feat * dfeat.double()).sum().backward()
        big, dres = guarded(N * T, D, dtype)
        dg, db = torch.full((D,), float("nan"), device="cuda"), torch.full((D,), float("nan"), device="cuda")
        ops.probe_pool_bwd(x.cuda(), dfeat.cuda(), gamma.cuda(), dres.view(N, T, D), dg, db, gp)
        what = f"pool bwd gp={gp} T={T} D={D} N={N} {dtype}"
        assert_close(dres.view(N, T, D), xd.grad, rt, at, what)
        assert guards_intact(big)
        assert not bool(dres.view(N, T, D)[:, 0 if gp else 1:1 if gp else T].float().abs().sum() > 0), "rows outside the pool must be zero"
        assert_close(dg, gd.grad, *GRAD, what + " dgamma")
        assert_close(db, bd.grad, *GRAD, what + " dbeta")
        ops.probe_pool_bwd(x.cuda(), dfeat.cuda(), gamma.cuda(), dres.view(N, T, D), dg, db, gp, accumulate=True)
        assert_close(dg, 2 * gd.grad, *GRAD, what + " dgamma accumulated")
        assert_close(db, 2 * bd.grad, *GRAD, what + " dbeta accumulated")
        assert_close(dres.view(N, T, D), xd.grad, rt, at, what + " (dres is written, never accumulated)")


def test_probe_pool_bwd_refuses_a_mean_over_nothing_before_any_launch(ops):
    x, w = torch.zeros(2, 1, 128), torch.ones(128)   # CPU tensors: the refusal comes before the pointer check, let alone a launch
    with pytest.raises(ValueError, match="nothing to average"):
        ops.probe_pool_bwd(x, torch.zeros(2, 128), w, torch.zeros(2, 1, 128), w.clone(), w.clone(), True)
    xg, wg = x.cuda(), w.cuda()
    dres = torch.full((2, 1, 128), float("nan"), device="cuda")
    ops.probe_pool_bwd(xg, torch.ones(2, 128, device="cuda"), wg, dres, wg.clone(), wg.clone(), False)   # the cls token alone is fine
    assert bool(torch.isfinite(dres).all())


# ------------------------------------------------------------------------------------------------ targets, soft cross-entropy, classifier dX
@pytest.mark.parametrize("N", [1, 3, 128])
@pytest.mark.parametrize("K", [2, 5, 62, 1000])
def test_mixup_target_soft_ce_and_head_dx_vs_fp64(ops, K, N):
    logits, labels = _ce_case(N, K, seed=7 * N + K)
    gout = 0.7
    for lam in (0.0, 0.3, 1.0):
        for smoothing in (0.0, 0.1):
            what = f"N={N} K={K} lam={lam} s={smoothing}"
            bigt, tgt = guarded(N, K)
            ops.mixup_target(labels.cuda(), tgt, lam=lam, smoothing=smoothing)
            ref_t = R.mixup_target_ref(labels, K, lam, smoothing)
            assert_close(tgt, ref_t, *VAL, "target " + what)
            assert_close(tgt.sum(1), torch.ones(N), *VAL, "target rows sum to 1 " + what)
            assert guards_intact(bigt)
            lr = logits.double().requires_grad_(True)
            ref = R.soft_ce_ref(lr, tgt.double().cpu())   # (against the targets the loss kernel reads)
            (ref * gout).backward()
            loss = torch.full((1,), float("nan"), device="cuda")
            bigd, dl = guarded(N, K)
            ops.soft_ce(logits.cuda(), tgt.contiguous(), loss, dlogits=dl, gout=torch.tensor([gout], device="cuda"))
            assert_close(loss[0], ref, *VAL, "soft ce " + what)
            assert_close(dl, lr.grad, *GRAD, "soft ce dlogits " + what)
            assert guards_intact(bigd)
            ops.soft_ce(logits.cuda(), tgt.contiguous(), loss)   # no gradient asked for
            assert_close(loss[0], ref, *VAL, "soft ce, loss only " + what)
    # lam = 1 is plain label smoothing, and on one-hot targets the soft loss is the hard one
    t1, ts = torch.empty(N, K, device="cuda"), torch.empty(N, K, device="cuda")
    ops.mixup_target(labels.cuda(), t1, lam=1.0, smoothing=0.1)
    assert_close(t1, R.smooth_one_hot(labels, K, 0.9 + 0.1 / K, 0.1 / K), *VAL, "lam = 1 equals smoothing")
    ops.mixup_target(labels.cuda(), ts, lam=1.0, smoothing=0.0)
    assert torch.equal(ts.cpu(), F.one_hot(labels, K).float())
    soft, hard = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    ops.soft_ce(logits.cuda(), ts, soft)
    ops.softmax_ce(logits.cuda(), labels.cuda(), hard)
    assert_close(soft, hard, *VAL, "soft ce on one-hot targets vs softmax_ce")
    # classifier dX from a gradient of the size the loss produces, with and without the upstream scale
    D = 200
    w = rnd(K, D, seed=N + K + 1, scale=0.1)
    d = lr.grad
    bigx, dx = guarded(N, D)
    ops.head_linear_dx(d.float().cuda(), w.cuda(), dx)
    assert_close(dx, d.float().double() @ w.double(), *GRAD, f"head dX N={N} K={K}")
    ops.head_linear_dx(d.float().cuda(), w.cuda(), dx, gscale=torch.tensor([0.5], device="cuda"))
    assert_close(dx, 0.5 * (d.float().double() @ w.double()), *GRAD, "head dX scaled")
    assert guards_intact(bigx)


def test_mixup_target_out_of_range_label_indexes_nothing(ops):
    N, K = 4, 5
    labels = torch.tensor([1, 4, 0, 2])
    for bad in (K, -1, 2 ** 40):
        lab = labels.clone()
        lab[2] = bad
        big, tgt = guarded(N, K)
        ops.mixup_target(lab.cuda(), tgt, lam=0.3, smoothing=0.1)
        assert guards_intact(big)
        assert_close(tgt, R.mixup_target_ref(lab, K, 0.3, 0.1), *VAL, f"label {bad}")


# ------------------------------------------------------------------------------------------------ mixup / cutmix of the images
@pytest.mark.parametrize("S", [16, 30, 15])   # 30: vectors straddle image rows; 15: C H W is no multiple of 4, the scalar variant
@pytest.mark.parametrize("N", [2, 6])
def test_mixup_cutmix_is_exact(ops, N, S):
    x = rnd(N, 3, S, S, seed=N + S)
    for lam in (0.0, 0.37, 1.0):
        big, out = guarded(N, 3 * S * S)
        ops.mixup_cutmix(x.cuda(), out.view(N, 3, S, S), lam=lam)
        assert torch.equal(out.view(N, 3, S, S).cpu(), R.mix_images_ref(x, lam)), f"mixup lam={lam}"
        assert guards_intact(big)
    boxes = [(4, 4, 2, 9), (0, S, 0, S), (2, 9, 3, 8), (0, 5, 1, 6), (S - 4, S, 2, 7), (3, 8, 0, 5), (1, 6, S - 3, S)]
    for box in boxes:   # empty, whole image, odd xl with an odd width, then a box on the top / bottom / left / right border
        big, out = guarded(N, 3 * S * S)
        ops.mixup_cutmix(x.cuda(), out.view(N, 3, S, S), box=box)
        assert torch.equal(out.view(N, 3, S, S).cpu(), R.mix_images_ref(x, box=box)), f"cutmix box={box}"
        assert guards_intact(big)


def test_mixup_cutmix_refuses_an_odd_batch_before_any_launch(ops):
    x = torch.zeros(3, 3, 16, 16)   # CPU tensors: refused before the pointer check
    with pytest.raises(ValueError, match="even"):
        ops.mixup_cutmix(x, torch.zeros_like(x), lam=0.5)


# ------------------------------------------------------------------------------------------------ position-embedding gradient
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [128, 768])
@pytest.mark.parametrize("T", [5, 17])
@pytest.mark.parametrize("N", [1, 4])
def test_pos_embed_grad_vs_fp64_sum(ops, N, T, D, dtype):
    dres = rnd(N, T, D, seed=N + T + D, scale=0.1).to(dtype)
    ref = dres.double().sum(0)
    big, dpos = guarded(T, D)
    ops.pos_embed_grad(dres.cuda(), dpos)
    assert_close(dpos, ref, *GRAD, f"dpos N={N} T={T} D={D} {dtype}")
    ops.pos_embed_grad(dres.cuda(), dpos, accumulate=True)
    assert_close(dpos, 2 * ref, *GRAD, "dpos accumulated")
    assert guards_intact(big)


# ------------------------------------------------------------------------------------------------ fine-tune steps, end to end
# AdamW's eps: the update g / (|g| + eps) turns round-off on a gradient that is zero by construction (the key bias: softmax does not see it)
# into steps of either sign, so with torch's default 1e-8 the CPU restatement in float32 misses the parameter bar against ITSELF in float64 by
# a factor 130 - 800 on blocks.*.attn.qkv.bias; with 1e-3 its own float32 error is 1.5 % of the bar (1e-4: 15 %), and gradients of 1e-3 .. 1e-2
# still take genuinely Adam-shaped steps.  Both optimizers get the same eps.
N_FT, K_FT, LR_FT, EPS_FT = 4, 5, 1e-3, 1e-3
GRAD_BAR = (2e-3, 2e-4)   # rtol, atol x scale: the gradient bar of test_micro_variants_fp32_vs_reference_and_oracle
BF16_LOSS_RTOL = 2e-3     # the bf16 loss bar of test_full_size_vitb_224_n128_vs_reference (tests/test_model_gpu.py: BF16_LOSS_RTOL)
FT_STEPS = [dict(lam=0.6, box=None), dict(lam=0.6, box=None), dict(lam=None, box=(10, 42, 21, 53))]   # fixed draws: mixup twice, then one cutmix box


def build_finetune_pair(global_pool):
    """(model for the chip, its CPU twin with identical parameters): micro trunk weights, non-trivial final norm and head."""
    import copy
    import models_vit
    from util.checkpoint_keys import to_vit_keys
    vit = models_vit.vit_base_patch16(num_classes=K_FT, global_pool=global_pool, **VIT_MICRO)
    sd = {k: v.float() for k, v in to_vit_keys(R.micro_sd()).items()}
    norm = "fc_norm" if global_pool else "norm"
    sd[norm + ".weight"], sd[norm + ".bias"] = 1 + 0.1 * rnd(128, seed=8), 0.1 * rnd(128, seed=9)
    sd["head.weight"], sd["head.bias"] = rnd(K_FT, 128, seed=10, scale=0.05), rnd(K_FT, seed=11, scale=0.05)
    if global_pool:
        sd.pop("norm.weight"), sd.pop("norm.bias")
    vit.load_state_dict(sd, strict=True)
    vit.finetune_mode()
    return vit, copy.deepcopy(vit)


def lrd_optimizer(model, cls, lr=LR_FT, eps=None):
    import util.lr_decay as lrd
    groups = lrd.param_groups_lrd(model, 0.05, no_weight_decay_list=model.no_weight_decay(), layer_decay=0.75)
    assert len(groups) == 2 * (len(model.blocks) + 2)
    opt = cls(groups, lr=lr, eps=EPS_FT if eps is None else eps)
    for g in opt.param_groups:   # what lr_sched.adjust_learning_rate does with a constant schedule
        g["lr"] = lr * g["lr_scale"]
    return opt


def step_inputs(step):
    imgs, labels = rnd(N_FT, 3, 64, 64, seed=20 + step), torch.tensor([0, 3, 3, 1])
    d = FT_STEPS[step]
    lam = d["lam"]
    if d["box"] is not None:
        yl, yh, xl, xh = d["box"]
        lam = 1.0 - (yh - yl) * (xh - xl) / (64.0 * 64.0)
    return imgs, labels, lam, d["box"]


def reference_run(twin, global_pool, dtype=torch.float32, eps=None, steps=len(FT_STEPS)):
    """Three steps of the CPU restatement with torch.optim.AdamW on the layer-decay groups -> losses, first-step gradients, final parameters."""
    twin = twin.to(dtype)
    opt = lrd_optimizer(twin, torch.optim.AdamW, eps=eps)
    losses, grads = [], None
    for step in range(steps):
        imgs, labels, lam, box = step_inputs(step)
        x = R.mix_images_ref(imgs, lam if box is None else 1.0, box).to(dtype)
        target = R.mixup_target_ref(labels, K_FT, lam, 0.1, dtype=dtype)
        loss, _ = R.finetune_loss_ref(dict(twin.named_parameters()), x, target, global_pool)
        opt.zero_grad()
        loss.backward()
        if grads is None:
            grads = {n: p.grad.detach().clone() for n, p in twin.named_parameters()}
        opt.step()
        losses.append(float(loss))
    return losses, grads, {n: p.detach().clone() for n, p in twin.named_parameters()}


_REF = {}


def reference(global_pool):
    if global_pool not in _REF:
        _REF[global_pool] = reference_run(build_finetune_pair(global_pool)[1], global_pool)
    return _REF[global_pool]


def chip_run(vit, dtype, steps=len(FT_STEPS), eps=None):
    from csmae_hip.optim import FusedAdamW
    from util.mixup import Mixup
    vit.cuda().train()
    vit.compute_dtype = dtype
    mix = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1, num_classes=K_FT)
    opt, losses, grads = None, [], None
    for step in range(steps):
        imgs, labels, lam, box = step_inputs(step)
        x, target = mix.mix(imgs.cuda(), labels.cuda(), lam, box)
        loss, logits = vit(x, target)
        assert loss.requires_grad and not logits.requires_grad
        loss.backward()
        if opt is None:   # (the parameters are homed in the flat buffer by the first forward)
            opt = lrd_optimizer(vit, FusedAdamW, eps=eps)
        if grads is None:
            grads = {n: p.grad.detach().float().cpu().clone() for n, p in vit.named_parameters()}
        opt.step()
        opt.zero_grad()
        losses.append(float(loss))
    return losses, grads, {n: p.detach().float().cpu().clone() for n, p in vit.named_parameters()}


def assert_bar(got, want, what):
    bad = []
    for n, w in want.items():
        g, scale = got[n], float(w.abs().max())
        err = (g.double() - w.double()).abs()
        tol = GRAD_BAR[0] * w.double().abs() + GRAD_BAR[1] * scale + 1e-12
        print(f"{what} {n}: max|err| {float(err.max()):.3e}, scale {scale:.3e}, worst err/tol {float((err / tol).max()):.3f}")
        if not bool((err <= tol).all()):
            bad.append((n, float(err.max()), scale))
    assert not bad, (what, bad)


@pytest.mark.parametrize("global_pool", [True, False])
def test_three_finetune_steps_fp32_match_the_cpu_restatement(ops, global_pool):
    want_loss, want_grad, want_param = reference(global_pool)
    vit, _ = build_finetune_pair(global_pool)
    losses, grads, params = chip_run(vit, torch.float32)
    print("loss", losses, want_loss)
    assert set(grads) == set(want_grad) >= {"pos_embed", "cls_token", "patch_embed.proj.weight", "head.weight", "head.bias"}
    for a, b in zip(losses, want_loss):
        assert abs(a - b) <= LOSS_RTOL * abs(b), (losses, want_loss)
    assert_bar(grads, want_grad, "grad")
    assert_bar(params, want_param, "param after 3 steps")
    for n, p in vit.named_parameters():   # the gradients are views of the one flat buffer FusedAdamW steps
        assert p.grad is None and vit._flat.owner_of(p) is vit._flat, n


def test_one_step_at_adamw_default_eps_where_the_gradient_is_not_round_off(ops):
    """FusedAdamW over the layer-decay groups in Adam's usual regime (eps = 1e-8): one step, compared at the parameter bar on the elements whose
    reference gradient is at least ten times the gradient bar's absolute floor (2e-4 x scale), i.e. |g| >= 2e-3 x scale.  There a gradient
    within the bar keeps its sign and |g| >> eps, so the first step -lr g / (|g| + eps) differs by less than lr eps |dg| / g^2 — nothing;
    the elements left out are those where the step's sign rests on round-off (the key bias, zero by construction, among them)."""
    _, want_grad, want_param = reference_run(build_finetune_pair(True)[1], True, eps=1e-8, steps=1)
    vit, twin = build_finetune_pair(True)
    before = {n: p.detach().clone() for n, p in twin.named_parameters()}
    _, _, params = chip_run(vit, torch.float32, steps=1, eps=1e-8)
    bad, checked = [], 0
    for n, w in want_param.items():
        g = want_grad[n]
        mask = g.abs() >= 10 * GRAD_BAR[1] * float(g.abs().max())
        scale = float(w.abs().max())
        err = (params[n].double() - w.double()).abs()
        tol = GRAD_BAR[0] * w.double().abs() + GRAD_BAR[1] * scale + 1e-12
        checked += int(mask.sum())
        moved = float((w - before[n]).abs()[mask].min()) if bool(mask.any()) else 0.0
        print(f"{n}: {int(mask.sum())}/{mask.numel()} elements, worst err/tol {float((err / tol)[mask].max()) if bool(mask.any()) else 0.0:.3f}, smallest move {moved:.2e}")
        if bool((err > tol)[mask].any()):
            bad.append((n, float(err[mask].max()), scale))
    assert not bad, bad
    assert checked > 0.5 * sum(w.numel() for w in want_param.values()), "the mask must leave most of the model under test"


@pytest.mark.parametrize("global_pool", [True, False])
def test_finetune_step_bf16_tracks_the_cpu_restatement(ops, global_pool):
    want_loss, want_grad, _ = reference(global_pool)
    vit, _ = build_finetune_pair(global_pool)
    losses, grads, _ = chip_run(vit, torch.bfloat16, steps=1)
    print("loss", losses, want_loss[:1])
    assert abs(losses[0] - want_loss[0]) <= BF16_LOSS_RTOL * abs(want_loss[0])
    cos = {n: float(F.cosine_similarity(grads[n].reshape(1, -1).double(), w.reshape(1, -1).double())) for n, w in want_grad.items()}
    print("cosine", cos)
    assert all(c >= 0.98 for c in cos.values()), {n: c for n, c in cos.items() if c < 0.98}


def test_accumulation_reproducibility_and_generation_check(ops):
    """Two backward calls accumulate (fp32 engine: the sum of the two separate gradients within GRAD, elementwise), a repeated run gives the same bits, a backward after a second forward is refused.
    The bit-identity of an ACCUMULATING run is checked on the bf16 engine: the fp32 parity engine reduces its bias gradients with
    csmae_colsum, whose partial sums meet in float atomics — on top of a non-zero gradient their order shows (measured: blocks.0.attn.qkv.bias
    differed between two fp32 runs of two backward calls).  That kernel belongs to the pre-training step and is left as it is."""
    def grads_of(batches, dense, dtype=torch.float32):
        vit, _ = build_finetune_pair(True)
        vit.cuda().train()
        vit.compute_dtype = dtype
        vit.smoothing = 0.1
        for step in batches:
            imgs, labels, _, _ = step_inputs(step)
            target = labels.cuda()
            if dense:
                target = ops.mixup_target(target, torch.empty(N_FT, K_FT, device="cuda"), lam=0.6, smoothing=0.1)
            loss, _ = vit(imgs.cuda(), target)
            loss.backward()
        return vit, {n: p.grad.detach().clone() for n, p in vit.named_parameters()}
    _, g0 = grads_of([0], False)
    _, g1 = grads_of([1], False)
    vit, g01 = grads_of([0, 1], False)
    for n in g0:
        assert_close(g01[n], g0[n].double() + g1[n].double(), *GRAD, "accumulated " + n)
    _, again = grads_of([0], False)
    for n in g0:
        assert torch.equal(g0[n], again[n]), f"{n}: a repeated fp32 run must give the same bits"
    for dense in (False, True):
        _, b0 = grads_of([0, 1], dense, torch.bfloat16)
        _, b1 = grads_of([0, 1], dense, torch.bfloat16)
        for n in b0:
            assert torch.equal(b0[n], b1[n]), f"{n}: a repeated accumulating bf16 run must give the same bits (dense={dense})"
    # a backward after a second forward is refused: the workspace holds the second forward's activations
    imgs, labels, _, _ = step_inputs(0)
    first, _ = vit(imgs.cuda(), labels.cuda())
    second, _ = vit(imgs.cuda(), labels.cuda())
    with pytest.raises(RuntimeError, match="activations are gone"):
        first.backward()
    second.backward()
    with pytest.raises(RuntimeError):
        second.backward()


# ------------------------------------------------------------------------------------------------ command line
@pytest.fixture(scope="module")
def pretrain_checkpoint(tmp_path_factory):
    return write_pretrain_checkpoint(tmp_path_factory.mktemp("pretrain"))


def test_cli_synthetic_epoch_checkpoint_resume_and_eval(ops, pretrain_checkpoint, tmp_path):
    import main_finetune
    import models_vit
    import util.lr_decay as lrd
    import util.misc as misc
    from csmae_hip.optim import FusedAdamW
    flags = ["--dataset_type", "synthetic", "--epochs", "1", "--model", "vit_base_patch16", "--embed_dim", "128", "--depth", "2", "--num_heads", "2",
             "--input_size", "64", "--batch_size", "4", "--nb_classes", "5", "--synthetic_len", "3", "--warmup_epochs", "0", "--output_dir", str(tmp_path),
             "--device", "cuda"]
    cwd = os.path.join(ROOT, "cross-scale-mae_amd")
    run = subprocess.run([sys.executable, "main_finetune.py", "--finetune", pretrain_checkpoint, "--transform_checkpoint_keys"] + flags,
                         cwd=cwd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    path = tmp_path / "checkpoint-0.pth"
    assert path.exists() and (tmp_path / "log.jsonl").exists()
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    before = torch.load(pretrain_checkpoint, map_location="cpu", weights_only=False)["model"]
    assert not torch.equal(ckpt["model"]["blocks.0.attn.qkv.weight"], before["encoder.0.attn.qkv.weight"]), "the trunk must have moved"
    assert not torch.equal(ckpt["model"]["pos_embed"], before["encoder_pos_embed"]), "the position table must have moved"
    # what --resume does (main_finetune.main up to the epoch loop): model, layer-decay groups, FusedAdamW, misc.load_model
    args = main_finetune.get_args_parser().parse_args(flags + ["--resume", str(path)])
    vit = models_vit.vit_base_patch16(num_classes=5, global_pool=True, **VIT_MICRO).finetune_mode().cuda()
    opt = FusedAdamW(lrd.param_groups_lrd(vit, 0.05, no_weight_decay_list=vit.no_weight_decay(), layer_decay=0.75), lr=1e-3)
    misc.load_model(args=args, model_without_ddp=vit, optimizer=opt, loss_scaler=None)
    assert args.start_epoch == 1
    own = vit.state_dict()
    for k, v in ckpt["model"].items():
        assert torch.equal(own[k].cpu(), v), k
    state = ckpt["optimizer"]["state"]
    assert len(state) == len(list(vit.parameters())) and len(ckpt["optimizer"]["param_groups"]) == 8
    for i, p in enumerate(q for g in opt.param_groups for q in g["params"]):
        assert torch.equal(opt.state[p]["exp_avg"].cpu(), state[i]["exp_avg"]) and float(state[i]["step"]) == 3, i
    assert sum(float(s["exp_avg"].abs().max()) > 0 for s in state.values()) >= len(state) - 2
    ev = subprocess.run([sys.executable, "main_finetune.py", "--eval", "--resume", str(path)] + flags, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stdout[-2000:] + ev.stderr[-2000:]
    assert "acc1:" in ev.stdout and "macro_f1:" in ev.stdout, ev.stdout[-1000:]
    # ... and through main itself: a second epoch from the checkpoint
    more = subprocess.run([sys.executable, "main_finetune.py", "--resume", str(path)] + [f if f != "1" or flags[i - 1] != "--epochs" else "2" for i, f in enumerate(flags)],
                          cwd=cwd, capture_output=True, text=True, timeout=300)
    assert more.returncode == 0, more.stdout[-2000:] + more.stderr[-2000:]
    assert "With optim & sched!" in more.stdout and "Epoch: [1]" in more.stdout and "Epoch: [0]" not in more.stdout
    second = torch.load(tmp_path / "checkpoint-1.pth", map_location="cpu", weights_only=False)
    assert second["epoch"] == 1 and all(float(st["step"]) == 6 for st in second["optimizer"]["state"].values())
    assert not torch.equal(second["model"]["head.weight"], ckpt["model"]["head.weight"])
