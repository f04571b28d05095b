"""The reference's eval transform (util/datasets.py:140-158) restated from torchvision 0.15's documented rules, for the tests of the GPU
input step: `ToTensor -> Normalize -> Resize(int(S / crop_pct), bicubic, antialias) -> CenterCrop(S)`.  Nothing here imports the code
under test (util/gpu_input.py), so the parameter table, the float64 chain and the explicit weight matrices are independent of it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# H, W, S -> Hr, Wr, top, left
PARAM_TABLE = {
    (97, 120, 64): (73, 90, 4, 13),
    (300, 260, 224): (295, 256, 36, 16),
    (225, 1000, 224): (256, 1137, 16, 456),
    (512, 400, 256): (327, 256, 36, 0),
    (33, 47, 32): (36, 51, 2, 10),
    (64, 64, 64): (73, 73, 4, 4),
}


def eval_geometry(H, W, S):
    """(Hr, Wr, top, left): Resize(int) maps the shorter side to `size` and the longer to int(size * long / short); CenterCrop starts at
    int(round((Hr - S) / 2.0)) with Python's round."""
    crop_pct = 224 / 256 if S <= 224 else 1.0
    size = int(S / crop_pct)
    short, long = (W, H) if W <= H else (H, W)
    new_short, new_long = size, int(size * long / short)
    Wr, Hr = (new_short, new_long) if W <= H else (new_long, new_short)
    return Hr, Wr, int(round((Hr - S) / 2.0)), int(round((Wr - S) / 2.0))


def eval_transform_ref(img_u8_hwc, mean, std, S, dtype=torch.float64):
    """[C, S, S] in `dtype` on the CPU: what the reference's eval Compose gives for one decoded image (tensor Resize is
    torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=True))."""
    H, W, C = img_u8_hwc.shape
    Hr, Wr, top, left = eval_geometry(H, W, S)
    x = img_u8_hwc.permute(2, 0, 1).to(dtype) / 255
    m, s = torch.as_tensor(mean, dtype=dtype).reshape(C, 1, 1), torch.as_tensor(std, dtype=dtype).reshape(C, 1, 1)
    x = (x - m) / s
    x = F.interpolate(x[None], size=(Hr, Wr), mode="bicubic", align_corners=False, antialias=True)[0]
    return x[:, top:top + S, left:left + S].contiguous()


def cubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def axis_weights(n_in, n_out):
    """[n_out, n_in] float64: row o holds the renormalised anti-aliased bicubic weights of output o (scale = in / out, centre =
    scale * (o + 0.5), support = 2 * max(scale, 1), taps clipped to [0, in))."""
    scale = n_in / n_out
    support, inv = (2.0 * scale, 1.0 / scale) if scale >= 1.0 else (2.0, 1.0)
    M = np.zeros((n_out, n_in), dtype=np.float64)
    for o in range(n_out):
        c = scale * (o + 0.5)
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)
        w = np.array([cubic((k - c + 0.5) * inv) for k in range(lo, hi)])
        M[o, lo:hi] = w / w.sum()
    return M


def eval_transform_matrices(img_u8_hwc, mean, std, S):
    """The same chain by explicit per-axis weight matrices in numpy float64: rows top..top+S of Wy, rows left..left+S of Wx."""
    H, W, C = img_u8_hwc.shape
    Hr, Wr, top, left = eval_geometry(H, W, S)
    x = img_u8_hwc.numpy().astype(np.float64).transpose(2, 0, 1) / 255
    x = (x - np.asarray(mean, dtype=np.float64).reshape(C, 1, 1)) / np.asarray(std, dtype=np.float64).reshape(C, 1, 1)
    Wy, Wx = axis_weights(H, Hr)[top:top + S], axis_weights(W, Wr)[left:left + S]
    return np.matmul(np.matmul(Wy, x), Wx.T)


def random_image(H, W, C, seed):
    return torch.randint(0, 256, (H, W, C), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def write_png_dataset(root, n, classes, seed, name):
    """n random RGB PNGs with sides in [40, 90] under root/name/ + root/name.csv (label, path; every other path relative to the CSV).
    -> (csv path, list of uint8 HWC tensors, labels)."""
    import os

    from PIL import Image
    g = torch.Generator().manual_seed(seed)
    os.makedirs(os.path.join(root, name), exist_ok=True)
    images, labels, rows = [], [], ["category,image_path"]
    for i in range(n):
        h, w = (int(v) for v in torch.randint(40, 91, (2,), generator=g))
        im = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
        rel = os.path.join(name, f"{i}.png")
        Image.fromarray(im.numpy()).save(os.path.join(root, rel))
        images.append(im)
        labels.append(i % classes)
        rows.append(f"{i % classes},{rel if i % 2 else os.path.join(root, rel)}")
    csv = os.path.join(root, f"{name}.csv")
    with open(csv, "w") as f:
        f.write("\n".join(rows) + "\n")
    return csv, images, labels


assert math.isclose(cubic(0.0), 1.0) and cubic(1.0) == 0.0 and cubic(2.0) == 0.0
