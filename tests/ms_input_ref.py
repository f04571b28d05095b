"""What the multispectral input tests share: seeded 13-band uint16 tiles, a TIFF writer built on `struct` (independent of util/tiff.py), and the
float64 oracle of the reference's EuroSAT transform chain (util/datasets.py:489-564 with BaseDataset.build_transform, :108-158), written with
torch's CPU `interpolate` and without a look at the kernel source."""
import struct
import zlib

import numpy as np
import torch

BANDS = 13
# util/datasets.py:490-519 (restated here so that the oracle does not read the code under test)
MEAN = np.array([1370.19151926, 1184.3824625, 1120.77120066, 1136.26026392, 1263.73947144, 1645.40315151, 1846.87040806, 1762.59530783, 1972.62420416,
                 582.72633433, 14.77112979, 1732.16362238, 1247.91870117])
STD = np.array([633.15169573, 650.2842772, 712.12507725, 965.23119807, 948.9819932, 1108.06650639, 1258.36394548, 1233.1492281, 1364.38688993,
                472.37967789, 14.3114637, 1310.36996126, 1087.6020813])


def tile(seed, H, W, C=BANDS):
    """uint16 [H, W, C] over the whole range of the type."""
    return np.random.default_rng(seed).integers(0, 65536, size=(H, W, C), dtype=np.uint16)


# ------------------------------------------------------------------------------------------------ TIFF writer
def write_tiff(path, arr, order="<", planar=False, compression=1, rows_per_strip=None, predictor=1, tiled=False, geo=True):
    """arr [H, W, C] uint8 / uint16 as a classic strip TIFF.  `compression` 8 deflates the strips; 5 (LZW), `predictor` 2 and `tiled` only set the
    tags (the payload is not valid for them: the reader must refuse before it looks).  `geo` adds a GeoTIFF tag the reader does not know."""
    H, W, C = arr.shape
    bits = arr.dtype.itemsize * 8
    rows = rows_per_strip or H
    raw = arr.astype(arr.dtype.newbyteorder(order))
    planes = [raw[:, :, c] for c in range(C)] if planar else [raw]
    strips = []
    for p in planes:
        for r0 in range(0, H, rows):
            b = np.ascontiguousarray(p[r0:r0 + rows]).tobytes()
            strips.append(zlib.compress(b) if compression in (8, 32946) else b)
    SHORT, LONG, DOUBLE = 3, 4, 12
    entries = [(256, LONG, [W]), (257, LONG, [H]), (258, SHORT, [bits] * C), (259, SHORT, [compression]), (262, SHORT, [1]), (277, SHORT, [C]),
               (278, LONG, [rows]), (284, SHORT, [2 if planar else 1]), (339, SHORT, [1] * C)]
    if predictor != 1:
        entries.append((317, SHORT, [predictor]))
    if geo:
        entries.append((33550, DOUBLE, [10.0, 10.0, 0.0]))   # ModelPixelScaleTag
    if tiled:
        entries += [(322, LONG, [16]), (323, LONG, [16]), (324, LONG, None), (325, LONG, [len(s) for s in strips])]
    else:
        entries += [(273, LONG, None), (279, LONG, [len(s) for s in strips])]
    entries.sort(key=lambda e: e[0])
    code = {SHORT: "H", LONG: "I", DOUBLE: "d"}
    ifd_at = 8
    extra_at = ifd_at + 2 + 12 * len(entries) + 4
    sizes = [struct.calcsize(code[t]) * (len(v) if v is not None else len(strips)) for _, t, v in entries]
    data_at = extra_at + sum(s for s in sizes if s > 4)
    offsets, at = [], data_at
    for s in strips:
        offsets.append(at)
        at += len(s)
    out = bytearray((b"II" if order == "<" else b"MM") + struct.pack(order + "HI", 42, ifd_at))
    out += struct.pack(order + "H", len(entries))
    extra = bytearray()
    for (tag, t, v), size in zip(entries, sizes):
        v = offsets if v is None else v
        packed = struct.pack(f"{order}{len(v)}{code[t]}", *v)
        out += struct.pack(order + "HHI", tag, t, len(v))
        if size <= 4:
            out += packed.ljust(4, b"\0")
        else:
            out += struct.pack(order + "I", extra_at + len(extra))
            extra += packed
    out += struct.pack(order + "I", 0) + extra
    assert len(out) == data_at
    for s in strips:
        out += s
    with open(path, "wb") as f:
        f.write(bytes(out))


# ------------------------------------------------------------------------------------------------ float64 oracle
def _normalised(tile_hwc, masked):
    x = torch.from_numpy(tile_hwc.astype(np.float64)).permute(2, 0, 1).clone()   # 1. float64 [C, H, W]
    for b in masked:
        x[b] = MEAN[b]                                                              # 2. masked bands := their mean
    return (x - torch.from_numpy(MEAN)[:, None, None]) / torch.from_numpy(STD)[:, None, None]   # 3. Normalize


def _resize(x, size):
    return torch.nn.functional.interpolate(x[None], size=size, mode="bicubic", antialias=True, align_corners=False)[0]


def oracle_train(tile_hwc, params, S, masked=(), dropped=()):
    """The training chain for one tile under params (H, W, i, j, h, w, hflip, vflip) -> float64 [Cout, S, S]."""
    H, W, i, j, h, w, hf, vf = params
    assert tile_hwc.shape[:2] == (H, W)
    x = _normalised(tile_hwc, masked)
    if hf:
        x = x.flip(-1)
    if vf:
        x = x.flip(-2)
    y = _resize(x[:, i:i + h, j:j + w].contiguous(), (S, S))
    assert y.dtype == torch.float64
    return y[[b for b in range(x.shape[0]) if b not in dropped]]


def oracle_eval(tile_hwc, params, S, masked=(), dropped=()):
    """The eval chain for one tile under params (H, W, Hr, Wr, top, left, 0, 0) -> float64 [Cout, S, S]."""
    H, W, Hr, Wr, top, left = params[:6]
    assert tile_hwc.shape[:2] == (H, W)
    y = _resize(_normalised(tile_hwc, masked), (Hr, Wr))[:, top:top + S, left:left + S]
    assert y.shape[1:] == (S, S)
    return y[[b for b in range(y.shape[0]) if b not in dropped]]


def plan(masked=(), dropped=()):
    """(band, mean fp32, inv_std fp32) as the kernels take them, built without util.ms_input."""
    kept = [b for b in range(BANDS) if b not in dropped]
    band = torch.tensor([b | (0x100 if b in masked else 0) for b in kept], dtype=torch.int32)
    return band, torch.tensor(MEAN[kept], dtype=torch.float32), torch.tensor(1.0 / STD[kept], dtype=torch.float32)
