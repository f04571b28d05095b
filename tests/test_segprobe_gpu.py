"""csrc/segment.hip against fp64 in guarded buffers, and the linear segmentation probe end to end.  Every operand and output of a kernel call lives
inside a larger allocation with sentinel padding on both sides (tests/seg_ref.py Guarded): after each launch the padding is intact, the inputs are
unchanged, no output element is left unwritten, and every element is within the bound seg_ref derives for it (fp32 rounding of the stated formula,
never a kernel's own output).  Each case prints its worst error / bound ratio (-s shows them).  Needs an MI355X."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import seg_ref as R
from finetune_ref import ROOT, VIT_MICRO, write_pretrain_checkpoint

pytestmark = pytest.mark.gpu
F32, BF, U8, I64 = torch.float32, torch.bfloat16, torch.uint8, torch.int64


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


def G(shape, dtype, fill=None):
    return R.Guarded(tuple(shape), dtype, "cuda", fill)


def settle(ins, outs):
    torch.cuda.synchronize()
    for name, (b, want) in ins.items():
        assert b.outside_intact(), f"{name}: written outside the view"
        assert torch.equal(b.t.cpu(), want), f"{name}: an input was changed"
    for name, b in outs.items():
        assert b.outside_intact(), f"{name}: written outside the view"
        assert b.unwritten() == 0, f"{name}: {b.unwritten()} elements left unwritten"


def within(worst, name, got, want, bound):
    n, msg, ratio = R.violations(got, want, bound)
    worst[name] = max(worst.get(name, 0.0), ratio)
    assert n == 0, f"{name}: {n} elements out of bound; {msg} (ratio {ratio:.3f})"


def run_ce(ops, pl, labels, dpl=True, conf_prior=None, pred=False, gscale=None):
    """One guarded seg_ce call -> dict of the outputs on the CPU"""
    N, Gc, _, K = pl.shape
    S = labels.shape[-1]
    b = dict(pl=G(pl.shape, F32, pl), labels=G(labels.shape, U8, labels), loss=G((1,), F32), count=G((1,), I64), scratch=G((ops.SEG_CE_SCRATCH_FLOATS,), F32))
    ins = dict(pl=(b["pl"], pl), labels=(b["labels"], labels))
    outs = dict(loss=b["loss"], count=b["count"])
    if dpl:
        outs["dpl"] = b["dpl"] = G(pl.shape, F32)
    if conf_prior is not None:
        b["conf"] = G((K, K), I64, conf_prior)
    if pred:
        outs["pred"] = b["pred"] = G((N, S, S), U8)
    if gscale is not None:
        b["gscale"] = G((1,), F32, torch.tensor([gscale]))
        ins["gscale"] = (b["gscale"], torch.tensor([gscale]))
    ops.seg_ce(b["pl"].t, b["labels"].t, b["loss"].t, b["count"].t, dpl=b["dpl"].t if dpl else None, conf=b["conf"].t if "conf" in b else None,
               scratch=b["scratch"].t, gscale=b["gscale"].t if "gscale" in b else None, pred=b["pred"].t if pred else None)
    settle(ins, outs)
    assert b["scratch"].outside_intact(), "scratch: written outside the view"
    if "conf" in b:
        assert b["conf"].outside_intact(), "conf: written outside the view"
    return {k: v.t.cpu() for k, v in b.items() if k not in ("pl", "labels", "scratch", "gscale")}


@pytest.mark.parametrize("pattern", R.PATTERNS)
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "N%d-G%d-p%d-K%d" % c)
def test_seg_ce_against_fp64(ops, case, pattern):
    N, Gc, p, K = case
    pl, labels = R.case_inputs(N, Gc, p, K, pattern)
    ref = R.ce_case_ref(N, Gc, p, K, pattern)
    prior = torch.randint(0, 1000, (K, K), generator=torch.Generator().manual_seed(K))
    worst = {}
    out = run_ce(ops, pl, labels, dpl=True, pred=True)
    assert int(out["count"]) == ref["count"]
    within(worst, "loss", out["loss"], ref["loss"].reshape(1), ref["b_loss"].reshape(1))
    within(worst, "dpl", out["dpl"], ref["dpl"], ref["b_dpl"])
    keep = ~ref["tie"]
    assert torch.equal(out["pred"].long()[keep], ref["arg"][keep]), "argmax map differs from fp64 away from near-ties"
    if ref["count"] == 0:   # the empty-batch convention: loss 0, gradient all zeros (torch gives NaN here)
        assert float(out["loss"]) == 0.0 and not bool(out["dpl"].any())
    # the confusion matrix, exactly, accumulated onto existing content; near-tie pixels (at most 0.1 %, test_segprobe_cpu) are left out of both sides
    assert float(ref["tie"].double().mean()) <= R.TIE_CAP
    outc = run_ce(ops, pl, R.conf_labels(labels, ref["tie"]), dpl=False, conf_prior=prior)
    assert torch.equal(outc["conf"], prior + ref["conf"]), "confusion matrix differs from the reference"
    print(f"seg_ce {case} {pattern}: count {ref['count']}, worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_seg_ce_gscale_and_no_gradient_side_effects(ops):
    N, Gc, p, K = 3, 3, 8, 21
    pl, labels = R.case_inputs(N, Gc, p, K, "ignore30")
    ref = R.ce_case_ref(N, Gc, p, K, "ignore30", gscale=-2.5)
    worst = {}
    out = run_ce(ops, pl, labels, dpl=True, gscale=-2.5)
    within(worst, "dpl", out["dpl"], ref["dpl"], ref["b_dpl"])
    within(worst, "loss", out["loss"], ref["loss"].reshape(1), ref["b_loss"].reshape(1))
    print("seg_ce gscale: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def test_seg_ce_conf_accumulates_over_calls(ops):
    N, Gc, p, K = 2, 2, 4, 5
    a, b = R.case_inputs(N, Gc, p, K, "random"), R.case_inputs(N, Gc, p, K, "ignore30", seed=1)
    zero = torch.zeros(K, K, dtype=I64)
    ca = run_ce(ops, *a, dpl=False, conf_prior=zero)["conf"]
    cb = run_ce(ops, *b, dpl=False, conf_prior=zero)["conf"]
    both = run_ce(ops, *b, dpl=False, conf_prior=ca)["conf"]
    assert torch.equal(both, ca + cb)
    assert int(ca.sum()) == N * (Gc * p) ** 2 and int(cb.sum()) == int((b[1] != R.IGNORE).sum())
    assert torch.equal(cb.sum(1), torch.bincount(b[1][b[1] != R.IGNORE].long(), minlength=K)), "rows are the true class"


@pytest.mark.parametrize("case", [(1, 14, 16, 16), (2, 4, 16, 64)], ids=lambda c: "N%d-G%d-p%d-K%d" % c)
def test_seg_ce_is_deterministic(ops, case):
    pl, labels = R.case_inputs(*case, "ignore30")
    a, b = run_ce(ops, pl, labels), run_ce(ops, pl, labels)
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32)) and torch.equal(a["dpl"].view(torch.int32), b["dpl"].view(torch.int32))


def test_seg_ce_stray_labels_stay_in_bounds(ops):
    """Labels in [K, 255) are the caller's contract; the kernels do not detect them, and they index nothing."""
    N, Gc, p, K = 2, 2, 4, 5
    pl, labels = R.case_inputs(N, Gc, p, K, "ignore30")
    labels = labels.clone()
    labels[0, ::3, ::2] = 254
    labels[1, 1::4, :] = K
    out = run_ce(ops, pl, labels, dpl=True, conf_prior=torch.zeros(K, K, dtype=I64), pred=True)
    assert int(out["count"]) == int((labels != R.IGNORE).sum()) and int(out["conf"].sum()) == int((labels < K).sum())
    assert bool(torch.isfinite(out["loss"]).all()) and bool(torch.isfinite(out["dpl"]).all())


@pytest.mark.parametrize("shape,why", [((1, 2, 2, 1, 8), "K = 1"), ((1, 2, 2, 65, 8), "K = 65"), ((1, 2, 2, 3, 10), "p = 5"), ((1, 3, 3, 3, 13), "S != G p")])
def test_seg_ce_refusals(ops, shape, why):
    import csmae_hip
    N, Gc, _, K, S = shape
    pl, labels = G((N, Gc, Gc, K), F32, torch.zeros(N, Gc, Gc, K)), G((N, S, S), U8, torch.zeros(N, S, S, dtype=U8))
    loss, count, dpl = G((1,), F32), G((1,), I64), G((N, Gc, Gc, K), F32)
    with pytest.raises(csmae_hip.CsmaeError):
        ops.seg_ce(pl.t, labels.t, loss.t, count.t, dpl=dpl.t)
    torch.cuda.synchronize()
    for b in (loss, count, dpl):   # refused before any launch: nothing was written
        assert b.outside_intact() and b.unwritten() == b.n, why


# ------------------------------------------------------------------------------------------------ LayerNorm of the patch tokens
# (N, T, D): one group / several groups / the widest vector form; D % 4 != 0 and D > 2048 take the scalar form; rows that are no multiple of a workgroup's 4
LN_SHAPES = ((2, 5, 128), (1, 17, 768), (2, 4, 2048), (3, 2, 70), (1, 3, 2052), (5, 4, 4))


@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", LN_SHAPES, ids=lambda s: "N%d-T%d-D%d" % s)
def test_seg_token_norm_against_fp64(ops, shape, dtype):
    N, T, D = shape
    x, gamma, beta = R.ln_inputs(N, T, D, dtype)
    want, bound = R.ln_ref(x, gamma, beta)
    bx, bg, bb, out = G(x.shape, dtype, x), G((D,), F32, gamma), G((D,), F32, beta), G((N * (T - 1), D), F32)
    ops.seg_token_norm(bx.t, bg.t, bb.t, out.t)
    settle(dict(x=(bx, x), gamma=(bg, gamma), beta=(bb, beta)), dict(out=out))
    worst = {}
    within(worst, "out", out.t, want, bound)
    print(f"seg_token_norm {shape} {dtype}: worst err / bound {worst['out']:.3f}")


def test_seg_token_norm_refusals(ops):
    import csmae_hip
    x, out = G((2, 1, 8), F32, torch.zeros(2, 1, 8)), G((1, 8), F32)
    with pytest.raises(csmae_hip.CsmaeError):   # T = 1: no patch row behind the cls row
        csmae_hip.check(csmae_hip.load().csmae_seg_token_norm(0, 2, 1, 8, x.t.data_ptr(), x.t.data_ptr(), x.t.data_ptr(), 1e-6, out.t.data_ptr(), None), "csmae_seg_token_norm")
    torch.cuda.synchronize()
    assert out.unwritten() == out.n and out.outside_intact()


# ------------------------------------------------------------------------------------------------ end to end
K_E2E = 3


@pytest.fixture(scope="module")
def e2e(ops):
    """A micro ViT under the probe, and 8 synthetic 64 x 64 images whose label is a fixed function of the patch's mean colour."""
    import models_seg
    import models_vit
    torch.manual_seed(0)
    vit = models_vit.vit_base_patch16(num_classes=2, global_pool=False, **VIT_MICRO)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        vit.norm.weight.copy_(1 + 0.1 * torch.randn(128, generator=g))
        vit.norm.bias.copy_(0.1 * torch.randn(128, generator=g))
    probe = models_seg.LinearSegProbe(vit.cuda(), K_E2E)
    colour = torch.randn(8, 4, 4, 3, generator=g)
    img = colour.repeat_interleave(16, 1).repeat_interleave(16, 2).permute(0, 3, 1, 2) + 0.1 * torch.randn(8, 3, 64, 64, generator=g)
    cls = (colour[..., 0] > 0).long() + (colour[..., 1] > 0).long()          # classes 0 / 1 / 2 with shares 1/4, 1/2, 1/4
    labels = cls.repeat_interleave(16, 1).repeat_interleave(16, 2).to(U8)
    labels[3, 5:12, 20:41] = R.IGNORE
    return probe, img.contiguous().cuda(), labels.contiguous().cuda()


def test_forward_patch_tokens_is_the_final_norm_of_the_stream(ops, e2e):
    probe, x, _ = e2e
    vit = probe.vit
    tok = vit.forward_patch_tokens(x)
    assert tok.shape == (8, 16, 128) and tok.dtype == F32
    stream = vit._engine(x).ws.enc["x"][len(vit.blocks)].view(8, 17, 128)
    want, bound = R.ln_ref(stream.cpu(), vit.norm.weight.detach().cpu(), vit.norm.bias.detach().cpu(), eps=vit.norm.eps)
    n, msg, ratio = R.violations(tok.reshape(128, 128), want, bound)
    assert n == 0, msg
    print(f"forward_patch_tokens: worst err / bound {ratio:.3f}")


def test_probe_head_gradient_and_frozen_trunk(ops, e2e):
    probe, x, labels = e2e
    probe.train()
    for p in probe.parameters():
        p.grad = None
    loss, pl = probe(x, labels)
    assert pl.shape == (8, 4, 4, K_E2E) and not pl.requires_grad and loss.requires_grad
    loss.backward()
    assert all(p.grad is None for p in probe.vit.parameters()), "the trunk is frozen"
    _, fbn = probe._logits(x)     # (training mode: batch statistics, the same rows the forward above fed the classifier)
    fbn64, plc, lab = fbn.double().cpu(), pl.detach().cpu(), labels.cpu()
    W = probe.linear.weight.detach().double().cpu().requires_grad_(True)
    b = probe.linear.bias.detach().double().cpu().requires_grad_(True)
    lin = (fbn64 @ W.t() + b).view(8, 4, 4, K_E2E)
    ref_loss = R.ce_loss(plc.double() + lin - lin.detach(), lab, 16)     # the kernel's own logits as values, the head's parameters as variables
    ref_loss.backward()
    ref = R.ce_ref(plc, lab, 16)
    within_ = {}
    within(within_, "loss", loss.detach().reshape(1), ref["loss"].reshape(1), ref["b_loss"].reshape(1))
    # dW = dpl^T fbn over a chain of R = 128 fused multiply-adds and one scaling; db = column sums of dpl over ceil(R / 64) + 8 additions
    u, rows = R.U32, fbn64.shape[0]
    d2, e2 = ref["dpl"].reshape(rows, K_E2E), ref["b_dpl"].reshape(rows, K_E2E)
    b_w = e2.t() @ fbn64.abs() + (rows + 2) * u * (d2.abs().t() @ fbn64.abs()) + 2 * u * W.grad.abs()
    b_b = e2.sum(0) + (-(-rows // 64) + 8) * u * d2.abs().sum(0) + 2 * u * b.grad.abs()
    within(within_, "dW", probe.linear.weight.grad, W.grad, b_w)
    within(within_, "db", probe.linear.bias.grad, b.grad, b_b)
    print("probe gradient: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in within_.items()))
    # a second backward accumulates
    g1 = probe.linear.weight.grad.clone()
    loss2, _ = probe(x, labels)
    (2.0 * loss2).backward()
    assert torch.allclose(probe.linear.weight.grad, 3.0 * g1, rtol=1e-5, atol=1e-9)


def test_twenty_probe_steps_lower_the_loss(ops, e2e):
    from util.lars import LARS
    probe, x, labels = e2e
    probe.train()
    for p in probe.parameters():
        p.grad = None
    # momentum 0: plain steps on the bias (LARS leaves vectors unscaled) descend the convex loss monotonically for lr < 2 / L, L <= 1 / 2
    opt = LARS(probe.head_parameters(), lr=0.5, weight_decay=0.0, momentum=0.0)
    losses = []
    for _ in range(20):
        loss, _ = probe(x, labels)
        opt.zero_grad(set_to_none=False)
        loss.backward()
        opt.step(gate=loss.detach().reshape(1))
        losses.append(loss.detach())
    losses = torch.stack(losses).cpu().tolist()
    print("probe losses: " + " ".join(f"{v:.4f}" for v in losses))
    assert losses[-1] < losses[0], (losses[0], losses[-1])


def test_probe_prediction_and_evaluation(ops, e2e):
    from util.metrics import miou_from_confusion
    probe, x, labels = e2e
    probe.eval()
    pred = probe(x)
    assert pred.shape == (8, 64, 64) and pred.dtype == U8
    loss, pl = probe(x, labels)
    ref = R.ce_ref(pl.cpu(), labels.cpu(), 16)
    keep = ~ref["tie"]
    assert torch.equal(pred.cpu().long()[keep], ref["arg"][keep])
    conf = torch.zeros(K_E2E, K_E2E, device="cuda", dtype=I64)
    l1, c1 = probe.evaluate_batch(x, labels, conf)
    l2, c2 = probe.evaluate_batch(x, labels, conf)
    valid = labels.cpu() != R.IGNORE
    assert int(c1) == int(c2) == int(valid.sum()) == ref["count"] and float(l1) == float(l2) == float(loss.detach())
    assert torch.equal(conf.cpu().sum(1), 2 * torch.bincount(labels.cpu()[valid].long(), minlength=K_E2E))
    assert float(ref["tie"].double().mean()) > 0 or torch.equal(conf.cpu(), 2 * ref["conf"])
    miou, per = miou_from_confusion(conf)
    assert 0.0 <= miou <= 1.0 and per.shape == (K_E2E,)


# ------------------------------------------------------------------------------------------------ command line
def test_cli_synthetic_two_epochs_log_checkpoints_and_eval(ops, tmp_path):
    """main_segprobe.main end to end in a child process: two epochs from the micro pre-training checkpoint, one log line and one checkpoint per
    epoch, then --eval --resume of the last checkpoint, whose mIoU is the last epoch's (an integer confusion matrix over the same seeded batches)."""
    ckpt = write_pretrain_checkpoint(tmp_path)
    out = tmp_path / "out"
    flags = ["--dataset_type", "synthetic", "--epochs", "2", "--save_every", "1", "--embed_dim", "128", "--depth", "2", "--num_heads", "2", "--input_size", "64",
             "--patch_size", "16", "--batch_size", "4", "--nb_classes", "3", "--synthetic_len", "4", "--output_dir", str(out), "--device", "cuda"]
    cwd = os.path.join(ROOT, "cross-scale-mae_amd")
    run = subprocess.run([sys.executable, "main_segprobe.py", "--finetune", ckpt, "--transform_checkpoint_keys"] + flags, cwd=cwd, capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    lines = [json.loads(ln) for ln in open(out / "log.txt")]
    assert [ln["epoch"] for ln in lines] == [0, 1]
    for ln in lines:   # (memory_alloc / time_epoch / time_step are the meters log_every adds)
        assert set(ln) == {"epoch", "train_loss", "train_lr", "train_memory_alloc", "train_time_epoch", "train_time_step", "test_loss", "test_mIoU", "test_pixel_acc", "test_iou"}, sorted(ln)
    for epoch in (0, 1):
        saved = torch.load(out / f"checkpoint-{epoch}.pth", map_location="cpu", weights_only=False)
        assert {"model", "optimizer", "epoch"} <= set(saved) and saved["epoch"] == epoch
    ev = subprocess.run([sys.executable, "main_segprobe.py", "--eval", "--resume", str(out / "checkpoint-1.pth")] + flags, cwd=cwd, capture_output=True, text=True,
                        timeout=300)
    assert ev.returncode == 0, ev.stdout[-2000:] + ev.stderr[-2000:]
    found = re.search(r"^\* mIoU ([0-9.]+)", ev.stdout, flags=re.M)
    assert found, ev.stdout[-1000:]
    print(f"segprobe cli: test_mIoU {lines[-1]['test_mIoU']!r}, --eval prints {found.group(1)}")
    assert found.group(1) == f"{lines[-1]['test_mIoU']:.3f}"
