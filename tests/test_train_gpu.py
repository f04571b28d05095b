"""End-to-end on the MI355X: the reference's config-1 epoch (BASELINE.json configs[0]) through our engine_pretrain loop, the CLI driver
with the synthetic loader, checkpoint round trip, and the data-parallel wrapper at world size 1 over RCCL."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def checksum(t):
    flat = t.double().reshape(-1).cpu()
    w = torch.arange(flat.numel(), dtype=torch.float64) % 97 + 1
    return [float(flat.sum()), float(flat.abs().sum()), float((flat * w).sum())]


def test_config1_epoch_matches_reference_engine():
    """MAE_ViT_Baseline ViT-B/16, 2x3x64x64, mask 0.75, one optimizer step: stats dict and updated weights vs the reference's
    engine_pretrain.train_one_epoch run on its CPU path (tests/golden/vitb_anchor.*)."""
    import models_mae
    from csmae_hip.optim import FusedAdamW, add_weight_decay
    from engine_pretrain import train_one_epoch
    from util.misc import NativeScalerWithGradNormCount
    a = json.load(open(os.path.join(G, "vitb_anchor.json")))
    d = np.load(os.path.join(G, "vitb_anchor.npz"))
    torch.manual_seed(0)
    m = models_mae.mae_vit_base(input_size=64, patch_size="16", loss="mse", device="cuda").cuda()
    m.compute_dtype = torch.float32  # parity mode (the loop itself runs under autocast like the reference's)
    opt = FusedAdamW(add_weight_decay(m, 0.05), lr=1e-3, betas=(0.9, 0.95))
    args = types.SimpleNamespace(accum_iter=1, lr=1e-3, min_lr=0.0, warmup_epochs=0, epochs=1, mask_ratio=0.75)
    m._test_draws = dict(noise=[torch.from_numpy(d["cfg1_noise"])], box=None)
    stats = train_one_epoch(m, [(torch.from_numpy(d["cfg1_imgs"]), None)], opt, torch.device("cuda"), 0, NativeScalerWithGradNormCount(), args=args)
    ref = a["cfg1_stats"]
    assert {"lr", "loss", "time_epoch", "time_step"} <= set(stats)
    assert stats["lr"] == ref["lr"]
    assert abs(stats["loss"] - ref["loss"]) < 1e-4 * abs(ref["loss"]), (stats["loss"], ref["loss"])
    sd = m.state_dict()
    for k, c in a["cfg1_after_checksums"].items():
        got = checksum(sd[k])
        for x, y in zip(got, c[:3]):
            assert abs(x - y) <= 2e-4 * abs(y) + 2e-3, (k, got, c[:3])


def test_cli_driver_synthetic_bf16_and_checkpoint(tmp_path):
    import main_pretrain
    argv = ["--model", "mae_vit_base_MsLdCeCd", "--dataset_type", "synthetic", "--input_size", "64", "--batch_size", "8", "--epochs", "2",
            "--warmup_epochs", "1", "--synthetic_len", "3", "--output_dir_base", str(tmp_path), "--output_dir", "run", "--blr", "1e-3"]
    args = main_pretrain.get_args_parser().parse_args(argv)
    main_pretrain.main(args)
    out = tmp_path / "run"
    logs = [json.loads(l) for l in open(out / "log.jsonl")]
    assert [l["epoch"] for l in logs] == [0, 1] and all(np.isfinite(l["train_loss"]) for l in logs)
    assert logs[1]["train_loss"] < logs[0]["train_loss"] + 0.5
    ck = torch.load(out / "checkpoint-1.pth", weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch", "scaler", "args"}
    assert "predictor.1.running_mean" in ck["model"] and len(ck["optimizer"]["state"]) > 200
    # resume: weights and AdamW moments come back
    args2 = main_pretrain.get_args_parser().parse_args(argv + ["--resume", str(out / "checkpoint-1.pth"), "--epochs", "3", "--honor_start_epoch"])
    main_pretrain.main(args2)
    logs = [json.loads(l) for l in open(out / "log.jsonl")]
    assert [l["epoch"] for l in logs] == [0, 1, 2]


def test_cli_driver_fmow_csv_through_gpu_input_step(tmp_path):
    """`--dataset_type fmow_rgb` reads the reference's CSV layout (label, path), decodes on the workers and runs the
    training transform on the GPU."""
    from PIL import Image
    import main_pretrain
    rng = np.random.default_rng(0)
    rows = ["label,image_path"]
    for k in range(12):
        h, w = 70 + 5 * k, 90 + 3 * k
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(tmp_path / f"im{k}.png")
        rows.append(f"{k % 3},im{k}.png")
    (tmp_path / "train.csv").write_text("\n".join(rows) + "\n")
    argv = ["--model", "mae_vit_base_MsLdCeCd", "--dataset_type", "fmow_rgb", "--train_path", str(tmp_path / "train.csv"), "--input_size", "64",
            "--batch_size", "4", "--epochs", "1", "--warmup_epochs", "0", "--num_workers", "0", "--output_dir_base", str(tmp_path), "--output_dir", "run"]
    main_pretrain.main(main_pretrain.get_args_parser().parse_args(argv))
    logs = [json.loads(l) for l in open(tmp_path / "run" / "log.jsonl")]
    assert len(logs) == 1 and np.isfinite(logs[0]["train_loss"])


def test_data_parallel_world1_rccl_matches_plain():
    import torch.distributed as dist
    import models_mae
    from csmae_hip.parallel import DataParallel
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29571")
    created = False
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        created = True
    try:
        micro = dict(dim_model=128, encoder_num_layers=6, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)
        x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
        g = torch.Generator().manual_seed(4)
        noise = [torch.rand(4, 16, generator=g), torch.rand(4, 16, generator=g)]
        grads = []
        for wrap in (False, True):
            torch.manual_seed(0)
            m = models_mae.MAE_ViT_MsLdCeCd(**micro, input_size=64, predictor_hidden_size=128).cuda()
            w = DataParallel(m) if wrap else m
            m._test_draws = dict(noise=noise, box=(7, 2, 45, 48))
            loss, _, _ = w(x)
            loss.backward()
            grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
        assert grads[0].keys() == grads[1].keys()
        for n in grads[0]:
            torch.testing.assert_close(grads[0][n], grads[1][n], rtol=1e-4, atol=1e-6)
        # Every bucket through a REAL RCCL all-reduce (world size 1 is a copy, but the launches, the side stream, the events against
        # the weight-gradient stream, the one-message buffer broadcast and the bf16 staging all run): the exchanged ranges tile the
        # flat gradient buffer incl. the update-gate slot exactly once, in gradient-ready order, and three optimizer steps end in
        # the same weights as the un-wrapped model (fp32 payload: bit-identical; bf16 payload: the gradients round once).
        from csmae_hip.optim import FusedAdamW, add_weight_decay
        finals = {}
        for mode in ("plain", "fp32", "bf16"):
            torch.manual_seed(0)
            m = models_mae.MAE_ViT_MsLdCeCd(**micro, input_size=64, predictor_hidden_size=128).cuda()
            m.compute_dtype = torch.bfloat16
            w = m if mode == "plain" else DataParallel(m, comm_dtype=None if mode == "fp32" else "auto", force_collectives=True)
            # (the wrapped runs step the way bench.py / main_pretrain.py do: the optimizer on its own stream behind the exchange's join, the next
            # forward pass ordering its layers behind the launch that steps their weights)
            opt = FusedAdamW(add_weight_decay(m, 0.05), lr=1e-3, betas=(0.9, 0.95), overlap=mode != "plain")
            gg = torch.Generator().manual_seed(9)
            for step in range(3):
                m._test_draws = dict(noise=[torch.rand(4, 16, generator=gg), torch.rand(4, 16, generator=gg)], box=(7, 2, 45, 48))
                opt.zero_grad(set_to_none=True)
                loss, _, _ = w(x)
                loss.backward()
                if mode != "plain":
                    sync, flat = w._sync, m._flat
                    ranges = sorted(sync.issued)
                    assert ranges[0][0] == 0 and ranges[-1][1] == flat.g.numel() and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:])), ranges
                    assert sync.issued[0] == w._ranges["tail"] and sync.issued[-1] == w._ranges["stem"] and len(sync.issued) == len(w._ranges)
                    assert (sync._staging is not None) == (mode == "bf16")
                    sync.issued.clear()
                opt.step()
            torch.cuda.synchronize()
            finals[mode] = {n: p.detach().clone() for n, p in m.named_parameters()}
        for n in finals["plain"]:
            assert torch.equal(finals["plain"][n], finals["fp32"][n]), n
            torch.testing.assert_close(finals["bf16"][n], finals["plain"][n], rtol=0, atol=4e-3)   # <= 3 steps of lr 1e-3 each
    finally:
        if created:
            dist.destroy_process_group()


def _dp_two_rank_worker(rank, world, port, out_dir):
    """Two processes on the ONE GPU of the test box, gloo as the transport (RCCL refuses two ranks on one device): exercises the
    world_size > 1 control flow of DataParallel + Engine.backward on real kernels — rank-0 broadcast, gradient-ready ranges,
    side-stream joins, BatchNorm buffer broadcast, no_sync."""
    import torch.distributed as dist
    import models_mae
    from csmae_hip.optim import FusedAdamW, add_weight_decay
    from csmae_hip.parallel import DataParallel
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        micro = dict(dim_model=128, encoder_num_layers=6, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)
        torch.manual_seed(100 + rank)  # different initial weights per rank: the wrapper must broadcast rank 0's
        m = models_mae.MAE_ViT_MsLdCeCd(**micro, input_size=64, predictor_hidden_size=128).cuda().train()
        w = DataParallel(m)
        opt = FusedAdamW(add_weight_decay(m, 0.05), lr=1e-3, betas=(0.9, 0.95))
        x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(10 + rank)).cuda()
        g = torch.Generator().manual_seed(20 + rank)
        grads = None
        for step in range(3):
            m._test_draws = dict(noise=[torch.rand(4, 16, generator=g), torch.rand(4, 16, generator=g)], box=(7, 2, 45, 48))
            opt.zero_grad(set_to_none=True)
            if step == 1:  # accumulation micro-step: no exchange, gradients stay local
                with w.no_sync():
                    loss, _, _ = w(x)
                    loss.backward()
                m._test_draws = dict(noise=[torch.rand(4, 16, generator=g), torch.rand(4, 16, generator=g)], box=(7, 2, 45, 48))
            loss, _, _ = w(x)
            loss.backward()
            if step == 0:
                grads = {n: p.grad.detach().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
            opt.step()
        torch.cuda.synchronize()
        torch.save(dict(params={n: p.detach().cpu() for n, p in m.named_parameters()}, grads=grads, loss=float(loss.detach()),
                        bn=m.predictor[1].running_mean.detach().cpu()), os.path.join(out_dir, f"rank{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_data_parallel_two_ranks_on_one_gpu_gloo(tmp_path):
    import torch.multiprocessing as mp
    port = 29600 + os.getpid() % 200
    mp.spawn(_dp_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert np.isfinite(r0["loss"]) and np.isfinite(r1["loss"])
    # gradients after the exchange are the mean over ranks -> identical on both; so are the parameters after three AdamW steps
    for n in r0["grads"]:
        torch.testing.assert_close(r0["grads"][n], r1["grads"][n], rtol=0, atol=0)
    for n in r0["params"]:
        torch.testing.assert_close(r0["params"][n], r1["params"][n], rtol=0, atol=0)
    # ... and they are not simply rank 0's local gradients: the two ranks saw different data
    m = max(float((r0["grads"][n]).abs().max()) for n in r0["grads"])
    assert m > 0


def test_bench_two_ranks_plumbing_on_one_gpu():
    """bench.py's N > 1 path exactly as the driver launches it (torch.distributed.run, one rank per process, barrier + max-over-ranks
    timing, rank 0 prints ONE JSON line) — with gloo and both ranks on the one GPU of the test box, because RCCL refuses two ranks on a
    device.  The 8-GPU RCCL run itself is the driver's."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, CSMAE_BENCH_ONE_GPU="1")
    port = 29700 + os.getpid() % 200
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", "2", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--batch", "8", "--no-kernel-timing", "--full"]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 2 and d["warmup"] == 1 and d["scaling"] == "weak" and d["config"]["global_batch"] == 16
    assert d["config"]["parallelism"] == "dp2" and d["value"] > 0 and np.isfinite(d["loss"]) and "cpu_baseline" not in d
    assert abs(d["value"] - 16 * 2 / (d["ms_per_step"] * 2 / 1e3)) < 1e-2 * d["value"]
    # the line verifies itself: both ranks took part, the replicas hold identical weights after the timed steps,
    # the ranks saw different data (different losses), every bucket went out, fp32 payload by default
    dp = d["data_parallel"]
    assert dp["ranks_seen"] == 2 and dp["weights_checksum_spread"] == 0.0 and dp["grad_payload"] == "fp32" and dp["buckets_per_step"] >= 3
    assert dp["ms_per_step_min"] <= dp["ms_per_step_max"] == d["ms_per_step"] and dp["loss_min"] < dp["loss_max"]
    # ... and diagnoses itself: the K steps once more without the collectives, per-bucket exchange times from events
    # on the exchange stream (one entry per bucket, tiling the flat gradient buffer + the gate slot), the RCCL knobs in force
    assert dp["ms_per_step_without_collectives"] > 0 and abs(dp["exposed_comm_ms"] - (d["ms_per_step"] - dp["ms_per_step_without_collectives"])) < 2e-3
    assert len(dp["bucket_allreduce"]) == dp["buckets_per_step"] and all(b["ms"] >= 0 and b["elements"] > 0 for b in dp["bucket_allreduce"])
    assert abs(dp["bucket_allreduce_ms_sum"] - sum(b["ms"] for b in dp["bucket_allreduce"])) < 1e-2
    assert dp["rccl_env"]["TORCH_NCCL_HIGH_PRIORITY"] == "1"


def test_bench_plain_line_and_dump_outputs(tmp_path):
    """A plain `bench.py --gpus 1` run: the headline line without the `--full` measurements, exactly --steps timed steps, and
    `--dump-outputs DIR` writing the last timed step's outputs as float32 .npy files (loss as in the line, mask, sampled prediction and
    updated weights) within 64 MB."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["unit"] == "images/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["ms_per_step"] > 0 and abs(d["value"] - 8 / (d["ms_per_step"] / 1e3)) < 1e-2 * d["value"]
    assert "cpu_baseline" not in d and "data_parallel" not in d and d["roofline"]["dominant_kernel"] is None and "clock_mhz_mean" not in d["chip"]
    files = sorted(os.listdir(tmp_path / "out"))
    assert files == ["loss.npy", "mask.npy", "params_sample.npy", "pred_sample.npy"], files
    arrs = {f[:-4]: np.load(tmp_path / "out" / f) for f in files}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
    assert abs(float(arrs["loss"][0]) - d["loss"]) <= 1e-4 * max(1.0, abs(d["loss"]))
    assert arrs["mask"].shape == (8, 196) and set(np.unique(arrs["mask"])) <= {0.0, 1.0} and int(arrs["mask"].sum()) == 8 * 147
    assert arrs["pred_sample"].size == 8 * 196 * 768 and arrs["params_sample"].size > 0


MICRO6 = dict(dim_model=128, encoder_num_layers=2, encoder_num_heads=2, decoder_embed_dim=64, decoder_num_layers=2, decoder_num_heads=2)


def _cecd(seed=0):
    import models_mae
    torch.manual_seed(seed)
    return models_mae.MAE_ViT_MsLdCeCd(**MICRO6, input_size=64, predictor_hidden_size=128).cuda().train()


def _draws(seed):
    g = torch.Generator().manual_seed(seed)
    return dict(noise=[torch.rand(4, 16, generator=g), torch.rand(4, 16, generator=g)], box=(7, 2, 45, 48))


def test_bf16_weight_mirror_follows_foreign_parameter_writes():
    """after the first bf16 forward, writes to the parameters that do not come from FusedAdamW — torch.optim.AdamW,
    load_state_dict, in-place edits — must reach the bf16 GEMM operands.  Each case is compared with a FRESH model holding the same
    fp32 weights (bit-identical bf16 forward: same kernels, same operands)."""
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()

    def fwd(m, seed=5):
        m.compute_dtype = torch.bfloat16
        m._test_draws = _draws(seed)
        return m(x)[0]

    def fresh_with(sd):
        f = _cecd(seed=99)
        f.load_state_dict(sd)
        return f

    m = _cecd()
    loss = fwd(m)
    loss.backward()
    # 1. torch.optim.AdamW steps the fp32 masters through torch ops
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=5e-2)
    opt.step()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    a, b = fwd(m.eval()), fwd(fresh_with(sd).eval())
    assert torch.equal(a, b), (float(a), float(b))
    assert abs(float(a) - float(loss)) > 1e-3 * abs(float(loss))  # (the step did change the function: a stale mirror would not see it)
    # 2. load_state_dict in the middle of a run
    other = {k: v.detach().clone() for k, v in _cecd(seed=7).state_dict().items()}
    m.load_state_dict(other)
    a, b = fwd(m), fwd(fresh_with(other).eval())
    assert torch.equal(a, b), (float(a), float(b))
    # 3. an in-place edit under no_grad
    with torch.no_grad():
        m.decoder_pred.weight.mul_(1.5)
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    a, b = fwd(m), fwd(fresh_with(sd).eval())
    assert torch.equal(a, b), (float(a), float(b))
    # 4. writes torch cannot see need the explicit mark
    m.decoder_pred.weight.data.mul_(0.5)
    m.mark_parameters_changed()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    a, b = fwd(m), fwd(fresh_with(sd).eval())
    assert torch.equal(a, b), (float(a), float(b))


def test_backward_belongs_to_its_forward():
    """the engine keeps one activation workspace.  A backward whose forward has been overwritten by a later
    forward, or that runs twice, raises; eval outputs are fresh tensors."""
    m = _cecd()
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    m._test_draws = _draws(1)
    l1 = m(x)[0]
    m._test_draws = _draws(2)
    l2 = m(x)[0]
    with pytest.raises(RuntimeError, match="activations are gone"):
        (l1 + l2).backward()
    m.zero_grad(set_to_none=True)
    m._test_draws = _draws(1)
    l1 = m(x)[0]
    with torch.no_grad():
        m.eval()
        m._test_draws = _draws(2)
        m(x)          # an evaluation forward between a training forward and its backward
        m.train()
    with pytest.raises(RuntimeError, match="activations are gone"):
        l1.backward()
    m._test_draws = _draws(1)
    l1 = m(x)[0]
    l1.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="twice"):
        l1.backward()
    # outside autograd the outputs do not alias the workspace
    with torch.no_grad():
        m._test_draws = _draws(1)
        _, pred1, mask1 = m(x)
        keep = pred1.clone()
        m._test_draws = _draws(2)
        _, pred2, _ = m(x)
    assert torch.equal(pred1, keep) and not torch.equal(pred1, pred2) and pred1.data_ptr() != pred2.data_ptr()


def test_clip_grad_norm_hip_matches_torch():
    """SURVEY §8 f-3 (util/misc.py:310-318): global-norm clipping on the flat gradient buffer (two HIP kernels, coefficient read on the
    device) against torch.nn.utils.clip_grad_norm_ on clones of the same gradients; norm-only mode against get_grad_norm_."""
    from util import misc
    m = _cecd()
    m.compute_dtype = torch.float32
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    m._test_draws = _draws(1)
    m(x)[0].backward()
    params = [p for p in m.parameters() if p.grad is not None]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for r, p in zip(ref, params):
        r.grad = p.grad.detach().clone()
    want_norm = torch.nn.utils.clip_grad_norm_(ref, 1e9)            # no clipping: the norm itself
    got = misc.clip_grad_norm_(m.parameters(), None)
    assert got.is_cuda and abs(float(got) - float(want_norm)) <= 2e-6 * float(want_norm)
    for r, p in zip(ref, params):
        assert torch.equal(r.grad, p.grad)                           # untouched
    max_norm = 0.37 * float(want_norm)
    want = torch.nn.utils.clip_grad_norm_(ref, max_norm)
    got = misc.clip_grad_norm_(m.parameters(), max_norm)
    assert abs(float(got) - float(want)) <= 2e-6 * float(want)
    for r, p in zip(ref, params):
        torch.testing.assert_close(p.grad, r.grad, rtol=2e-6, atol=0)
    after = misc.clip_grad_norm_(m.parameters(), None)
    assert abs(float(after) - max_norm) <= 1e-5 * max_norm
    # a larger bound leaves the gradients bit-identical (coefficient clamps to 1)
    before = [p.grad.clone() for p in params]
    misc.clip_grad_norm_(m.parameters(), 10.0 * float(after))
    assert all(torch.equal(a, p.grad) for a, p in zip(before, params))
    # the scaler contract routes through it
    m.zero_grad(set_to_none=True)
    from csmae_hip.optim import FusedAdamW, add_weight_decay
    opt = FusedAdamW(add_weight_decay(m, 0.05), lr=1e-3, betas=(0.9, 0.95))
    m._test_draws = _draws(1)
    norm = misc.NativeScalerWithGradNormCount()(m(x)[0], opt, clip_grad=max_norm, parameters=m.parameters())
    assert abs(float(norm) - float(want_norm)) <= 1e-4 * float(want_norm)


def test_clip_grad_norm_with_user_frozen_parameters_stays_on_the_flat_buffer():
    """util/misc.py:310-318 with part of the model frozen by the user: torch's clip_grad_norm_ norms only the parameters that have a
    gradient; the engine still writes dW / db of every layer into the flat buffer, so it clears the frozen slots at the end of the
    reverse pass and the two-kernel HIP path norms the buffer as a whole (no torch fallback)."""
    from csmae_hip.engine import FlatParams
    from util import misc
    m = _cecd()
    m.compute_dtype = torch.float32
    frozen = [n for n, _ in m.named_parameters() if n.startswith("encoder.0.") or n in ("decoder_pred.bias", "predictor.0.weight")]
    for n, p in m.named_parameters():
        if n in frozen:
            p.requires_grad_(False)
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()
    m._test_draws = _draws(1)
    m(x)[0].backward()
    named = dict(m.named_parameters())
    assert all(named[n].grad is None for n in frozen)
    flat = FlatParams.owner_of(named["decoder_pred.weight"])
    for n in frozen:   # the slots the kernels wrote are zero again
        assert float(flat.grad_views[n].abs().max()) == 0.0, n
    params = [p for p in m.parameters() if p.grad is not None]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for r, p in zip(ref, params):
        r.grad = p.grad.detach().clone()
    want_norm = torch.nn.utils.clip_grad_norm_(ref, 1e9)
    called = []
    orig = torch.nn.utils.clip_grad_norm_
    torch.nn.utils.clip_grad_norm_ = lambda *a, **k: called.append(1) or orig(*a, **k)
    try:
        got = misc.clip_grad_norm_(m.parameters(), None)
        max_norm = 0.5 * float(want_norm)
        want = orig(ref, max_norm)
        got2 = misc.clip_grad_norm_(m.parameters(), max_norm)
    finally:
        torch.nn.utils.clip_grad_norm_ = orig
    assert not called, "the frozen-parameter case fell back to torch"
    assert abs(float(got) - float(want_norm)) <= 2e-6 * float(want_norm) and abs(float(got2) - float(want)) <= 2e-6 * float(want)
    for r, p in zip(ref, params):
        torch.testing.assert_close(p.grad, r.grad, rtol=2e-6, atol=0)
    # a subset of the parameters (not the whole model) is still torch's business
    sub = [named["decoder_pred.weight"]]
    assert abs(float(misc.clip_grad_norm_(sub, None)) - float(sub[0].grad.norm())) <= 1e-6 * float(sub[0].grad.norm())


def test_gradient_clear_on_the_side_stream_is_ordered_against_every_main_stream_writer(monkeypatch):
    """the flat gradient buffer is cleared on the weight-gradient stream while the reconstruction head's backward runs on the
    main stream; main-stream writers into the buffer wait for that clear through ONE event.  A writer placed above the wait would race it
    and lose its contribution: the whole buffer must match the run whose clear sits on the main stream (CSMAE_DEBUG=zero_main), step after
    step — bit for bit where the step is bit-reproducible at this geometry (checked first: two default runs), to rounding otherwise."""
    from csmae_hip.engine import FlatParams
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()

    def run():
        m = _cecd()
        m.compute_dtype = torch.bfloat16
        snaps = []
        for k in range(3):
            m._test_draws = _draws(k + 1)
            m.zero_grad(set_to_none=True)
            m(x)[0].backward()
            flat = FlatParams.owner_of(m.decoder_pred.weight)
            snaps.append(flat.g.clone())
        run.slots = dict(flat.slots)
        return snaps
    side, side2 = run(), run()
    monkeypatch.setenv("CSMAE_DEBUG", "zero_main")
    main = run()
    reproducible = all(torch.equal(a, b) for a, b in zip(side, side2))
    for a, b in zip(side, main):
        if reproducible:
            assert torch.equal(a, b)
        else:   # (small shapes take kernels whose reduction order is not fixed: a lost contribution is orders of magnitude above that noise)
            #  per parameter slot, against that slot's own magnitude: a lost write into a small-magnitude slot (BatchNorm / LayerNorm
            # parameters, cls / mask tokens — the main- and auxiliary-stream writers this test is about) is far below 1e-3 of the GLOBAL maximum
            for name, (o, n, _) in run.slots.items():
                sa, sb = a[o:o + n], b[o:o + n]
                scale = float(sb.abs().max())
                assert float((sa - sb).abs().max()) <= 1e-3 * scale + 1e-12, (name, float((sa - sb).abs().max()), scale)


def test_serial_heads_match_the_overlapped_junction(monkeypatch):
    """the profiled / A-B path (CSMAE_DW_MAIN=1: every head on the main stream, the cross-decoder target gradient accumulated in
    fp32 by pair_loss_bwd) and the shipped step (predictor backward on the auxiliary stream, the target gradient added from the bf16 `dv` by
    rows_scatter_add2) compute the same gradients up to that one bf16 rounding of dv: every parameter slot within 2e-2 of its own maximum
    (measured: <= 4e-3), the loss identical."""
    from csmae_hip.engine import FlatParams
    x = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3)).cuda()

    def run():
        m = _cecd()
        m.compute_dtype = torch.bfloat16
        m._test_draws = _draws(7)
        m.zero_grad(set_to_none=True)
        loss = m(x)[0]
        loss.backward()
        flat = FlatParams.owner_of(m.decoder_pred.weight)
        torch.cuda.synchronize()
        return float(loss), flat.g[: flat.total].clone(), dict(flat.slots)
    l0, g0, slots = run()
    monkeypatch.setenv("CSMAE_DW_MAIN", "1")
    l1, g1, _ = run()
    assert l0 == l1
    for name, (o, n, _) in slots.items():
        a, b = g0[o:o + n], g1[o:o + n]
        scale = float(b.abs().max())
        assert float((a - b).abs().max()) <= 2e-2 * scale + 1e-12, (name, float((a - b).abs().max()), scale)


def test_non_finite_loss_never_reaches_the_weights():
    """ADVICE r1 (low) / engine_pretrain.py:56-58: the loop notices a non-finite loss only at its next drain; until then the fused
    optimizer must not apply the poisoned steps (device-side gate), and the drain raises."""
    import types
    from csmae_hip.optim import FusedAdamW, add_weight_decay
    from engine_pretrain import train_one_epoch
    from util.misc import NativeScalerWithGradNormCount
    m = _cecd()
    opt = FusedAdamW(add_weight_decay(m, 0.05), lr=1e-2, betas=(0.9, 0.95))
    good = torch.randn(4, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    bad = good.clone()
    bad[1, 0, 5, 5] = float("nan")
    args = types.SimpleNamespace(accum_iter=1, lr=1e-2, min_lr=0.0, warmup_epochs=0, epochs=1, mask_ratio=0.75)
    # one good step, then state snapshot
    train_one_epoch(m, [(good, None)], opt, torch.device("cuda"), 0, NativeScalerWithGradNormCount(), args=args)
    with pytest.raises(ValueError, match="stopping training"):
        train_one_epoch(m, [(good, None), (bad, None), (bad, None), (good, None)], opt, torch.device("cuda"), 0, NativeScalerWithGradNormCount(), args=args)
    # steps 1 (nan), 2 (nan) were skipped on the device; the mirror and the moments are finite
    for k, v in m.named_parameters():   # (BatchNorm running statistics are updated by the forward itself, in the reference too)
        assert torch.isfinite(v.float()).all(), k
    assert torch.isfinite(m._flat.w_lp.float()).all()
    for i, s in opt.state_dict()["state"].items():
        assert torch.isfinite(s["exp_avg"]).all() and torch.isfinite(s["exp_avg_sq"]).all()
    # and a model that only ever saw the good batches through the same loop agrees wherever the comparison is exact: the gate
    # makes a NaN step a no-op, so [good] + [good, nan, nan, good] == [good] + [good, good] up to the step counter's bias
    # correction (the host counter still advances) -- check finiteness + that training continues
    m._test_draws = _draws(1)
    loss = m(good.cuda())[0]
    assert torch.isfinite(loss)


def test_short_training_runs_track_the_fp32_engine():
    """Loss parity over optimizer steps, not only at step 0: ViT-B/16 MsLdCeCd at 64^2, 8 images, 12 fused-AdamW steps on the same draws
    in the three numerics modes.  The bf16 MFMA path (bf16 residual stream, 8-bit gelu', grouped weight gradients) and the fp8 path
    (delayed scaling from the second step on) must follow the exact-fp32 engine's loss trajectory and end at weights close to its."""
    import models_mae
    from csmae_hip.optim import FusedAdamW, add_weight_decay
    x = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(11)).cuda()
    runs = {}
    for mode in (torch.float32, torch.bfloat16, "fp8"):
        torch.manual_seed(0)
        m = models_mae.mae_vit_base_MsLdCeCd(input_size=64, patch_size="16", loss="mse", device="cuda").cuda().train()
        m.compute_dtype = mode
        opt = FusedAdamW(add_weight_decay(m, 0.05), lr=2e-4, betas=(0.9, 0.95))
        g = torch.Generator().manual_seed(12)
        losses = []
        for step in range(12):
            m._test_draws = dict(noise=[torch.rand(8, 16, generator=g), torch.rand(8, 16, generator=g)], box=(5 + step, 3, 40, 44))
            opt.zero_grad(set_to_none=True)
            loss, _, _ = m(x, mask_ratio=0.75)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        runs[mode] = (losses, {n: p.detach().float().clone() for n, p in m.named_parameters() if p.requires_grad})
    ref_l, ref_p = runs[torch.float32]
    assert ref_l[-1] < ref_l[0]                                            # it trains
    for mode, ltol, ptol in ((torch.bfloat16, 2e-3, 0.03), ("fp8", 1e-2, 0.12)):   # measured: 1.4e-4 / 0.050 and 2.0e-3 / 0.29
        losses, params = runs[mode]
        worst = max(abs(a - b) / abs(b) for a, b in zip(losses, ref_l))
        assert worst < ltol, (mode, worst, losses, ref_l)
        # weights after 12 steps: relative distance to the fp32 run, measured on the updates (AdamW moves every weight by ~lr per step)
        num = sum(float((params[n] - ref_p[n]).pow(2).sum()) for n in ref_p)
        torch.manual_seed(0)
        init = {n: p.detach().float().cuda() for n, p in models_mae.mae_vit_base_MsLdCeCd(input_size=64, patch_size="16", loss="mse", device="cpu").named_parameters() if p.requires_grad}
        den = sum(float((ref_p[n] - init[n]).pow(2).sum()) for n in ref_p)
        assert (num / den) ** 0.5 < ptol * 12 ** 0.5, (mode, (num / den) ** 0.5)
        print(f"[train 12 steps {mode}] worst loss deviation {worst:.2e}, update distance {(num / den) ** 0.5:.3f}")
