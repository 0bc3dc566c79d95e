"""Cycle-consistency quality of a CycleGAN on the device.  The translation G(x) of an unpaired set has no
ground truth, but the cycle has: F(G(x)) against x, G(F(y)) against y, and the identity maps F(x) against x and G(y) against y are
model-free figures, measured with gan_image_quality (SSIM as tf.image.ssim, PSNR, MAE).

`cycle_quality` chains the eval calls of the two generators on img_size batches - the typed output view of one call is copied into
the typed input of the next (gan_copy_view): no unpack and repack through fp32, no host round trip.  `cycle_quality_tiled` does the
same at the source resolution: the blended fp32 image of the first generator is cut into the second one's tiles by gan_tile_gather.
Both only enqueue; the rows stay on the device (quality.QualityMeter) until the caller drains them.  The inference forward writes no
state.  The reference has no such measurement."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import tiling
from .quality import image_quality

METRICS = ('ssim', 'psnr', 'mae')             # the first three columns of gan_image_quality's rows
GROUPS_X, GROUPS_Y = ('cycle_x', 'identity_x'), ('cycle_y', 'identity_y')


def keys(groups=GROUPS_X + GROUPS_Y):
    """Column names of the rows: cycle_x_ssim, cycle_x_psnr, cycle_x_mae, identity_x_ssim, ..."""
    return tuple(f'{g}_{m}' for g in groups for m in METRICS)


def _dense(ctx, x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return torch.as_tensor(x).to(device=ctx.device, dtype=torch.float32).contiguous()


def _one_side(ctx, first, second, x):
    """-> [B, 6]: the metrics of second(first(x)) against x, then those of second(x) against x."""
    B, S = x.shape[0], x.shape[1]
    a, b = first.eval_call(B, S), second.eval_call(B, S)
    a.set_input(x)
    a.infer(fold=False)
    src, dst = a.out_view(), b.xin.view(0, b.C)
    L.check(ctx.lib.gan_copy_view(ctx.dt, C.byref(src), C.byref(dst), ctx.stream()), "copy_view")
    b.infer(fold=False)
    cycle = image_quality(ctx, b.out_view(), x)
    b.set_input(x)
    b.infer(fold=False)
    same = image_quality(ctx, b.out_view(), x)
    return torch.cat([cycle[:, :3], same[:, :3]], dim=1)


def cycle_quality(model, x, y=None):
    """model: a CycleGAN whose generators were folded since the weights last changed (generator_g.fold(), generator_f.fold());
    x (and y): img_size batches, NHWC in [-1, 1].  -> float32 device tensor [B, 6] in the order keys(GROUPS_X): F(G(x)) against x,
    F(x) against x; with y [B, 12] in the order keys(): then G(F(y)) against y, G(y) against y.  A row depends on its own image
    only.  Enqueue-only on the current stream."""
    ctx, G, F = model.ctx, model.generator_g, model.generator_f
    rows = _one_side(ctx, G, F, _dense(ctx, x))
    if y is None:
        return rows
    return torch.cat([rows, _one_side(ctx, F, G, _dense(ctx, y))], dim=1)


def cycle_quality_tiled(model, src_u8, *, tile, overlap, batch=None):
    """The cycle at the source resolution.  src_u8: uint8 device image [H, W, C], H and W >= tile.  -> (rows, fake, cycled): the
    float32 device tensor [1, 3] = keys(('cycle_x',)) of F(G(x)) against the normalised source, and the two blended fp32 images
    [H, W, C].  Normalisation statistics stay per tile in both passes."""
    ctx, G, F = model.ctx, model.generator_g, model.generator_f
    fake = tiling.infer_tiled(G, src_u8, tile=tile, overlap=overlap, batch=batch, fold=False)
    cycled = tiling.infer_tiled(F, fake, tile=tile, overlap=overlap, batch=batch, fold=False)
    real = tiling.normalize_lut(ctx)[src_u8.long()]
    return image_quality(ctx, cycled[None], real[None])[:, :3], fake, cycled
