"""EuroSAT multispectral tiles (13-band Sentinel-2, uint16) as an input step on the GPU: the reference's `Dataset_eurosat`
(util/datasets.py:489-564 with build_fmow_dataset:597-607).

The reference reads a text file of `path label` lines, opens each tile as float64, overwrites `--masked_bands` with the band's mean, runs the
fMoW-RGB transform chain on the raw values (Dataset_eurosat defines no build_transform and inherits BaseDataset's, :108-158; ToTensor does not
divide a float array by 255) and removes `--dropped_bands` from the result.  Here the loader workers only read the tiles (`util.tiff.read_tiff`
or `.npy`); the uint16 values go to the device through the pinned double buffer of `util.gpu_input.GpuAugment` and one HIP kernel
(`csmae_augment_u16` / `csmae_eval_u16`, csrc/multispectral.hip) does masking, normalisation, flips, the antialiased bicubic crop or resize and
the band selection.  The random decisions and the eval geometry come from the same host functions as for RGB (`sample_transform_params`,
`eval_transform_params`), so a seeded run draws what the reference's transform would."""
from __future__ import annotations

import os
from typing import List, Optional, Sequence, Tuple

import torch

from util.gpu_input import GpuAugment, PackedBatch, PrefetchLoader, eval_transform_params, sample_transform_params

EUROSAT_BANDS = 13
EUROSAT_MEAN = (1370.19151926, 1184.3824625, 1120.77120066, 1136.26026392, 1263.73947144, 1645.40315151, 1846.87040806, 1762.59530783,
                1972.62420416, 582.72633433, 14.77112979, 1732.16362238, 1247.91870117)   # util/datasets.py:490-504
EUROSAT_STD = (633.15169573, 650.2842772, 712.12507725, 965.23119807, 948.9819932, 1108.06650639, 1258.36394548, 1233.1492281,
               1364.38688993, 472.37967789, 14.3114637, 1310.36996126, 1087.6020813)      # util/datasets.py:505-519
BAND_MASKED = 0x100      # bit 8 of a `band` entry (include/csmae.h csmae_augment_u16)
MAX_ROW_VALUES = 12288   # MS_MAX_ROW_FLOATS of csrc/multispectral.hip: Wmax * bands the kernel stages per source row


def band_plan(masked_bands: Optional[Sequence[int]], dropped_bands: Optional[Sequence[int]]) -> Tuple[List[int], List[float], List[float]]:
    """(band, mean, inv_std) of the kernels for `--masked_bands` / `--dropped_bands`: one entry per band that is kept, in band order; a masked
    band carries BAND_MASKED.  Raises ValueError for an index outside 0..12, a band both masked and dropped, or no band left."""
    masked, dropped = sorted(set(masked_bands or ())), sorted(set(dropped_bands or ()))
    for name, idx in (("masked_bands", masked), ("dropped_bands", dropped)):
        bad = [b for b in idx if not 0 <= b < EUROSAT_BANDS]
        if bad:
            raise ValueError(f"--{name} {bad}: EuroSAT bands are numbered 0..{EUROSAT_BANDS - 1}")
    both = sorted(set(masked) & set(dropped))
    if both:
        raise ValueError(f"bands {both} are both in --masked_bands and in --dropped_bands")
    kept = [b for b in range(EUROSAT_BANDS) if b not in dropped]
    if not kept:
        raise ValueError("--dropped_bands drops all 13 bands")
    band = [b | (BAND_MASKED if b in masked else 0) for b in kept]
    return band, [EUROSAT_MEAN[b] for b in kept], [1.0 / EUROSAT_STD[b] for b in kept]


def eurosat_channels(args) -> int:
    """The model's input channels for `--dataset_type euro_sat`: 13 - len(dropped_bands) (util/datasets.py:539-540).  An `--input_channels`
    that says otherwise raises ValueError."""
    n = len(band_plan(getattr(args, "masked_bands", None), getattr(args, "dropped_bands", None))[0])
    given = getattr(args, "input_channels", None)
    if given is not None and given != n:
        raise ValueError(f"--dataset_type euro_sat with --dropped_bands {getattr(args, 'dropped_bands', None)} has {n} bands: --input_channels {given} does not fit")
    return n


class EuroSatDataset(torch.utils.data.Dataset):
    """Text file with one `path label` per line (util/datasets.py:530-533); relative paths are taken against the list's folder.  `.tif` / `.tiff`
    are read by util.tiff.read_tiff, `.npy` holds [H, W, 13] uint16.  Returns (uint16 HWC tensor, label); no transform runs on the CPU."""

    def __init__(self, list_path: str):
        self.base = os.path.dirname(os.path.abspath(list_path))
        with open(list_path, "r") as f:
            rows = [ln.split() for ln in f.read().splitlines() if ln.strip()]
        self.paths, self.labels = [r[0] for r in rows], [int(r[1]) for r in rows]

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        import numpy as np
        p = self.paths[i]
        p = p if os.path.isabs(p) else os.path.join(self.base, p)
        if p.lower().endswith((".tif", ".tiff")):
            from util.tiff import read_tiff
            arr = read_tiff(p)
        elif p.lower().endswith(".npy"):
            arr = np.load(p)
        else:
            raise ValueError(f"{p}: EuroSAT tiles are read from .tif / .tiff / .npy files")
        if arr.ndim != 3 or arr.shape[2] != EUROSAT_BANDS:
            raise ValueError(f"{p}: a EuroSAT tile has {EUROSAT_BANDS} bands [H, W, {EUROSAT_BANDS}], this file holds an array of shape {tuple(arr.shape)}")
        if arr.dtype != np.uint16:
            if arr.dtype != np.uint8:
                raise ValueError(f"{p}: a EuroSAT tile holds uint16 values, this file holds {arr.dtype}")
            arr = arr.astype(np.uint16)
        return torch.from_numpy(np.ascontiguousarray(arr)), self.labels[i]


def pack_uint16(images) -> PackedBatch:
    """Tiles of one batch in one uint16 tensor [N, Hmax, Wmax, C] (tile n in the top-left corner) + their sizes [N, 2]: pack_uint8's counterpart."""
    N, C = len(images), int(images[0].shape[2])
    Hmax, Wmax = max(int(im.shape[0]) for im in images), max(int(im.shape[1]) for im in images)
    data = torch.zeros(N, Hmax, Wmax, C, dtype=torch.uint16)
    for n, im in enumerate(images):
        data[n, : im.shape[0], : im.shape[1]] = im
    return PackedBatch(data, torch.tensor([[int(im.shape[0]), int(im.shape[1])] for im in images], dtype=torch.int32))


def collate_uint16(samples):
    """DataLoader collate_fn: reading AND packing run in the worker processes; the main process copies once."""
    return pack_uint16([s[0] for s in samples]), torch.as_tensor([s[1] for s in samples])


class MsAugment(GpuAugment):
    """uint16 HWC tiles of 13 bands -> normalised fp32 [N, in_chans, S, S] on `device`: GpuAugment's staging protocol (pinned double buffer, copy
    stream, `stage` / `finish`) and host parameter functions around the u16 kernels.  `band`, `mean` and `inv_std` are built once."""

    def __init__(self, input_size: int, masked_bands=None, dropped_bands=None, device="cuda", train: bool = True, scale=(0.25, 1.0), slots: int = 2):
        band, mean, inv_std = band_plan(masked_bands, dropped_bands)
        super().__init__(input_size, mean=mean, std=[1.0 / v for v in inv_std], scale=scale, device=device, slots=slots, train=train)
        self.inv_std = torch.tensor(inv_std, dtype=torch.float32, device=self.device)   # (the plan's 1 / std, rounded to fp32 once)
        self.band = torch.tensor(band, dtype=torch.int32)   # on the host: the library checks it before each launch

    @property
    def in_chans(self) -> int:
        return int(self.band.numel())

    def stage(self, images, params: Optional[List[Tuple[int, ...]]] = None):
        """GpuAugment.stage for uint16 tiles: `images` is a list of uint16 HWC tensors / arrays or a PackedBatch from collate_uint16."""
        from csmae_hip import ops
        if not isinstance(images, PackedBatch):
            images = pack_uint16([torch.as_tensor(im) for im in images])
        N, Hmax, Wmax, C = images.data.shape
        if images.data.dtype != torch.uint16 or C != EUROSAT_BANDS:
            raise ValueError(f"MsAugment takes uint16 tiles of {EUROSAT_BANDS} bands, got {images.data.dtype} with {C}")
        if Wmax * C > MAX_ROW_VALUES:
            raise ValueError(f"a tile {Wmax} pixels wide does not fit the {MAX_ROW_VALUES} values per source row the kernel stages")
        nbytes = images.data.numel() * 2
        if params is None:
            if self.train:
                params = [sample_transform_params(int(h), int(w), self.scale) for h, w in images.sizes.tolist()]
            else:   # (raises before anything is enqueued when a tile is too large for the kernel)
                params = [eval_transform_params(int(h), int(w), self.S) for h, w in images.sizes.tolist()]
        s = self._slot(nbytes, N, self.in_chans)
        s["host"][:nbytes].view(torch.uint16).view(N, Hmax, Wmax, C).copy_(images.data)
        s["meta_host"][:N] = torch.tensor(params, dtype=torch.int32)
        self.copy_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.copy_stream):
            s["dev"][:nbytes].copy_(s["host"][:nbytes], non_blocking=True)
            s["meta_dev"][:N].copy_(s["meta_host"][:N], non_blocking=True)
            s["staged"] = torch.cuda.Event()
            s["staged"].record(self.copy_stream)
            src = s["dev"][:nbytes].view(torch.uint16).view(N, Hmax, Wmax, C)
            (ops.augment_u16 if self.train else ops.eval_u16)(src, s["meta_dev"][:N], self.band, self.mean, self.inv_std, s["out"][:N],
                                                              st=self.copy_stream.cuda_stream)
            ready = torch.cuda.Event()
            ready.record(self.copy_stream)
        return dict(slot=s, N=N, ready=ready)


def eurosat_loader(dataset, sampler, is_train: bool, args, device) -> PrefetchLoader:
    """`dataset` (an EuroSatDataset or a Subset of one) behind `sampler`: whole batches and the training transform, or the ragged last batch kept
    and the eval transform.  Uses args.batch_size / input_size / num_workers / masked_bands / dropped_bands."""
    raw = torch.utils.data.DataLoader(dataset, sampler=sampler, batch_size=args.batch_size, num_workers=args.num_workers, pin_memory=False,
                                      drop_last=is_train, collate_fn=collate_uint16)
    return PrefetchLoader(raw, MsAugment(args.input_size, getattr(args, "masked_bands", None), getattr(args, "dropped_bands", None), device=device,
                                         train=is_train))


def build_eurosat_loader(list_path: str, is_train: bool, args, device) -> PrefetchLoader:
    """The EuroSAT loader of the downstream drivers, as build_fmow_rgb_loader: train shuffled, eval in order; `len(loader.dataset)` is the number
    of tiles."""
    dataset = EuroSatDataset(list_path)
    sampler = torch.utils.data.RandomSampler(dataset) if is_train else torch.utils.data.SequentialSampler(dataset)
    return eurosat_loader(dataset, sampler, is_train, args, device)
