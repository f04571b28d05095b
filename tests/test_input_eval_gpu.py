"""The eval transform on the GPU (`csmae_eval_u8`, util/gpu_input.py) against the float64 chain of tests/input_eval_ref.py, its memory
guards, the exact identity case, the double-buffered eval loader, and both downstream drivers on a small PNG dataset.

Bar of the kernel per image: max|err| <= max(2e-4, 2 * e32).  2e-4 is the bar the training kernel meets on the same arithmetic
(test_ops_gpu.py::test_augment_u8_matches_reference_transform_chain); e32 is the error of the same chain run by torch in float32 against
float64, computed here for that image: torch's own fp32 position arithmetic degrades with the coordinate size."""
import argparse
import os
import subprocess
import sys

import pytest
import torch

import input_eval_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(97, 120), (300, 260), (64, 64), (512, 400), (33, 47), (225, 1000)]
VIT_MICRO = dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2)


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import csmae_hip
    from csmae_hip import ops as o
    csmae_hip.load()
    return o


def statistics(C):
    from util.gpu_input import FMOW_RGB_MEAN, FMOW_RGB_STD
    return list(FMOW_RGB_MEAN) + [0.4] * (C - 3), list(FMOW_RGB_STD) + [0.2] * (C - 3)


def run_eval_u8(ops, data, sizes, S, mean, std):
    """-> (dst [N, C, S, S] on the CPU, the whole guarded buffer on the CPU): dst is a view inside a NaN-filled buffer, one row each side."""
    from util.gpu_input import eval_transform_params
    N, C = data.shape[0], data.shape[3]
    meta = torch.tensor([eval_transform_params(h, w, S) for h, w in sizes], dtype=torch.int32).cuda()
    buf = torch.full((N + 2, C, S, S), float("nan"), device="cuda")
    m = torch.tensor(mean, dtype=torch.float32).cuda()
    ops.eval_u8(data.cuda(), meta, m, 1.0 / torch.tensor(std, dtype=torch.float32).cuda(), buf[1:-1])
    torch.cuda.synchronize()
    buf = buf.cpu()
    return buf[1:-1], buf


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("S", [32, 64, 224, 256])
def test_eval_u8_matches_the_float64_chain(ops, S, C):
    from util.gpu_input import pack_uint8
    mean, std = statistics(C)
    imgs = [R.random_image(h, w, C, seed=1000 * S + 10 * n + C) for n, (h, w) in enumerate(SIZES)]
    packed = pack_uint8(imgs)
    out, buf = run_eval_u8(ops, packed.data, SIZES, S, mean, std)
    assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[-1]).all()), "a guard row was written"
    assert not bool(torch.isnan(out).any())
    # the padding of the packed source is never read: 255 there gives the same bits as 0
    data255 = torch.full_like(packed.data, 255)
    for n, im in enumerate(imgs):
        data255[n, : im.shape[0], : im.shape[1]] = im
    out255, _ = run_eval_u8(ops, data255, SIZES, S, mean, std)
    assert torch.equal(out, out255), "bytes beyond an image's H x W reached its output"
    worst = (0.0, 0.0)
    for n, im in enumerate(imgs):
        ref = R.eval_transform_ref(im, mean, std, S, torch.float64)
        e32 = float((R.eval_transform_ref(im, mean, std, S, torch.float32).double() - ref).abs().max())
        err = float((out[n].double() - ref).abs().max())
        print(f"eval_u8 S={S} C={C} {SIZES[n][0]}x{SIZES[n][1]}: err {err:.3e}  e32 {e32:.3e}")
        worst = max(worst, (err, e32))
        assert err <= max(2e-4, 2 * e32), (S, C, SIZES[n], err, e32)
    print(f"eval_u8 S={S} C={C} worst (err, e32) = ({worst[0]:.3e}, {worst[1]:.3e})")


@pytest.mark.parametrize("S", [64, 224, 256])
def test_identity_resize_is_the_normalised_centre_crop(ops, S):
    """H == W == int(S / crop_pct): every window is one tap of weight cubic_aa(0) = 1 beside taps of weight cubic_aa(+-1) = 0."""
    from util.gpu_input import eval_transform_params
    mean, std = statistics(3)
    size = int(S / (224 / 256 if S <= 224 else 1.0))
    im = R.random_image(size, size, 3, seed=S)
    H, W, Hr, Wr, top, left, _, _ = eval_transform_params(size, size, S)
    assert (Hr, Wr) == (size, size) and top == left == int(round((size - S) / 2.0))
    out, _ = run_eval_u8(ops, im[None], [(size, size)], S, mean, std)
    # the kernel's inputs are the fp32 mean and 1 / std
    m32 = torch.tensor(mean, dtype=torch.float32)
    i32 = 1.0 / torch.tensor(std, dtype=torch.float32)
    crop = im[top:top + S, left:left + S].permute(2, 0, 1).double()
    want = (crop / 255 - m32.double().reshape(3, 1, 1)) * i32.double().reshape(3, 1, 1)
    err = float((out[0].double() - want).abs().max())
    print(f"identity S={S}: err {err:.3e}")
    assert err <= 1e-6, err


def test_eval_loader_double_buffering_and_ragged_last_batch(ops):
    from util.gpu_input import GpuAugment, PrefetchLoader, eval_transform_params, pack_uint8
    g = torch.Generator().manual_seed(9)
    counts = (4, 4, 2)
    batches = [([torch.randint(0, 256, (40 + 3 * k + i, 50 + k, 3), generator=g, dtype=torch.uint8) for i in range(n)], list(range(k, k + n)))
               for k, n in enumerate(counts)]
    aug = GpuAugment(32, train=False)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    got = [(x.cpu(), y) for x, y in PrefetchLoader(batches, aug)]
    assert torch.equal(torch.get_rng_state(), state), "the eval transform draws nothing"
    assert [x.shape[0] for x, _ in got] == list(counts)
    for (x, y), (imgs, labels) in zip(got, batches):
        assert y.dtype == torch.int64 and y.tolist() == labels
        packed = pack_uint8(imgs)
        meta = torch.tensor([eval_transform_params(int(h), int(w), 32) for h, w in packed.sizes.tolist()], dtype=torch.int32).cuda()
        want = torch.empty(len(imgs), 3, 32, 32, device="cuda")
        ops.eval_u8(packed.data.cuda(), meta, aug.mean, aug.inv_std, want)
        assert torch.equal(x, want.cpu())
    # an image the kernel cannot hold is refused on the host, before anything is enqueued
    with pytest.raises(ValueError, match="smaller size"):
        aug.stage([torch.zeros(900, 900, 3, dtype=torch.uint8)])


@pytest.fixture(scope="module")
def png_dataset(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("fmow_micro"))
    train_csv, _, _ = R.write_png_dataset(root, 12, 3, seed=21, name="train")
    val_csv, val_images, val_labels = R.write_png_dataset(root, 10, 3, seed=22, name="val")
    return dict(train=train_csv, val=val_csv, images=val_images, labels=val_labels)


@pytest.mark.parametrize("driver", ["main_linprobe", "main_finetune"])
def test_cli_rgb_epoch_then_eval(ops, driver, png_dataset, tmp_path):
    flags = ["--dataset_type", "rgb", "--train_path", png_dataset["train"], "--test_path", png_dataset["val"], "--model", "vit_base_patch16",
             "--embed_dim", "128", "--depth", "2", "--num_heads", "2", "--input_size", "64", "--batch_size", "4", "--nb_classes", "3", "--epochs", "1",
             "--warmup_epochs", "0", "--num_workers", "0", "--output_dir", str(tmp_path), "--device", "cuda"]
    cwd = os.path.join(ROOT, "cross-scale-mae_amd")
    run = subprocess.run([sys.executable, f"{driver}.py"] + flags, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    path = tmp_path / "checkpoint-0.pth"
    assert path.exists() and (tmp_path / "log.jsonl").exists()
    assert "Epoch: [0]  [2/3]" in run.stdout, run.stdout[-2000:]   # 12 images, whole batches of 4
    if driver == "main_finetune":
        assert "on the 10 test images" in run.stdout, run.stdout[-2000:]
    ev = subprocess.run([sys.executable, f"{driver}.py", "--eval", "--resume", str(path)] + flags, cwd=cwd, capture_output=True, text=True, timeout=300)
    assert ev.returncode == 0, ev.stdout[-2000:] + ev.stderr[-2000:]
    assert "Evaluation on 10 test images" in ev.stdout and "acc1:" in ev.stdout, ev.stdout[-1000:]


def test_evaluate_over_the_eval_loader_matches_the_reference_chain(ops, png_dataset):
    """The 10 validation images (4 + 4 + 2) through CsvImageDataset, two decoding workers and GpuAugment(train=False) give the same top-1
    count as the float32 reference chain fed to the same model."""
    import main_linprobe
    import models_vit
    from util.gpu_input import FMOW_RGB_MEAN, FMOW_RGB_STD, build_fmow_rgb_loader
    torch.manual_seed(4)
    vit = models_vit.vit_base_patch16(num_classes=3, global_pool=False, **VIT_MICRO).probe_mode()
    with torch.no_grad():
        vit.head[1].weight.normal_(std=0.05)   # (the probe head starts at std 2e-5: spread the logits)
    vit = vit.cuda()
    args = argparse.Namespace(batch_size=4, input_size=64, num_workers=2)
    loader = build_fmow_rgb_loader(png_dataset["val"], False, args, torch.device("cuda"))
    assert len(loader.dataset) == 10 and len(loader) == 3
    got = main_linprobe.evaluate(loader, vit, "cuda")
    images, labels = png_dataset["images"], png_dataset["labels"]
    ref_batches = [(torch.stack([R.eval_transform_ref(im, FMOW_RGB_MEAN, FMOW_RGB_STD, 64, torch.float32) for im in images[i:i + 4]]).cuda(),
                    torch.tensor(labels[i:i + 4])) for i in range(0, 10, 4)]
    want = main_linprobe.evaluate(ref_batches, vit, "cuda")
    assert got["acc1"] == want["acc1"], (got, want)
    assert abs(got["loss"] - want["loss"]) <= 1e-2 * abs(want["loss"]), (got, want)
