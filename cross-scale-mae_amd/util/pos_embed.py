"""2-D sin-cos positional table (reference util/pos_embed.py:16-63): float64 numpy, "w goes first", cls row = 0."""
import numpy as np


def get_2d_sincos_pos_embed(embed_dim, grid_size, cls_token=False):
    assert embed_dim % 4 == 0
    omega = 1.0 / 10000 ** (np.arange(embed_dim // 4, dtype=float) / (embed_dim / 4.0))
    hh, ww = np.divmod(np.arange(grid_size * grid_size), grid_size)
    aw, ah = np.outer(ww.astype(float), omega), np.outer(hh.astype(float), omega)
    table = np.concatenate([np.sin(aw), np.cos(aw), np.sin(ah), np.cos(ah)], axis=1)
    return np.concatenate([np.zeros([1, embed_dim]), table], axis=0) if cls_token else table


def interpolate_pos_embed(model, checkpoint_model, key="pos_embed"):
    """Resize a checkpoint's position table to the model's patch grid in place (reference util/pos_embed.py:72-97, after DeiT): the extra
    (cls) rows are kept, the grid rows are resampled bicubically.  A load-time host operation."""
    import torch
    if key not in checkpoint_model:
        return
    table = checkpoint_model[key]
    D = table.shape[-1]
    num_patches = model.patch_embed.num_patches
    extra = model.pos_embed.shape[-2] - num_patches
    old, new = int((table.shape[-2] - extra) ** 0.5), int(num_patches ** 0.5)
    if old == new:
        return
    print("Position interpolate from %dx%d to %dx%d" % (old, old, new, new))
    grid = table[:, extra:].reshape(-1, old, old, D).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid.float(), size=(new, new), mode="bicubic", align_corners=False)
    checkpoint_model[key] = torch.cat((table[:, :extra], grid.permute(0, 2, 3, 1).flatten(1, 2).to(table.dtype)), dim=1)
