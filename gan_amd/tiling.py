"""Prediction at the source resolution (include/gan_amd.h: gan_tile_grid / gan_tile_gather_u8 / gan_tile_blend; DESIGN.md section
13): an image larger than the network's input is cut into overlapping tiles on the device, the tiles go through the inference call
as one batch, and the outputs are blended back with hat weights - no fp32 staging tensor, no host round trip.

`tile_origins` / `tile_grid` restate the geometry in pure Python (the same rules as the C side; tests compare the two).  The
reference has no such path: it resizes every image to img_size x img_size before it predicts (pix2pix.py:43-52)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

MAX_SIDE = 4096


def _check_axis(L_, S, V):
    if S % 8 or not 16 <= S <= 1024:
        raise ValueError(f"tile size {S}: must be a multiple of 8 in [16, 1024]")
    if not 0 <= V <= S // 2:
        raise ValueError(f"tile overlap {V}: must lie in [0, {S // 2}] for tiles of {S}")
    if not S <= L_ <= MAX_SIDE:
        raise ValueError(f"image side {L_}: must lie in [{S}, {MAX_SIDE}] for tiles of {S} (nothing is padded)")


def tile_origins(L_, S, V):
    """Origins of the tiles along one axis of length L_: stride S - V, the last tile pulled back to end at the edge."""
    _check_axis(L_, S, V)
    T = S - V
    n = 1 if L_ == S else -(-(L_ - S) // T) + 1
    return [min(k * T, L_ - S) for k in range(n)]


def tile_grid(h, w, S, V):
    """-> (ny, nx): tiles per column / per row; tile t = ky * nx + kx has its origin at (tile_origins(h)[ky], tile_origins(w)[kx])."""
    return len(tile_origins(h, S, V)), len(tile_origins(w, S, V))


def normalize_lut(ctx):
    """The 256-entry table byte -> v / 127.5 - 1 on the context's device (one per context; the device dataset's table)."""
    if ctx.__dict__.get('_normalize_lut') is None:
        from .data import normalize_table
        ctx._normalize_lut = torch.from_numpy(normalize_table()).to(ctx.device)
    return ctx._normalize_lut


def gather_tiles(ctx, src_u8, dst_view, *, h, w, tile, overlap, t0, n, col0=0, lut=None, dtype=None):
    """Tiles [t0, t0 + n) of the h x w part of `src_u8` ([H, Wfull, C] uint8 on the device) that starts at column col0 ->
    `dst_view` (a GanTensor of n x tile x tile, C channels), normalised through `lut`.  Enqueue-only on the current stream."""
    H, wfull, c = src_u8.shape
    lut = normalize_lut(ctx) if lut is None else lut
    d = L.GanTileGatherDesc(ctx.dt if dtype is None else dtype, src_u8.data_ptr(), src_u8.numel(), wfull * c, col0, h, w, c, tile,
                            overlap, t0, n, lut.data_ptr(), dst_view)
    L.check(ctx.lib.gan_tile_gather_u8(C.byref(d), ctx.stream()), "tile_gather_u8")


_FLOAT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}


def gather_tiles_f(ctx, src, dst_view, *, h, w, tile, overlap, t0, n, col0=0, dtype=None):
    """gather_tiles from a float image (gan_tile_gather): `src` is an fp32 / bf16 / fp16 [H, Wfull, C] device tensor - the blended
    prediction of another generator - and no table is applied.  The destination's storage (`dtype`, default the context's) is the
    source's (a bit copy) or, for an fp32 source, any (rounded to nearest once).  Enqueue-only on the current stream."""
    H, wfull, c = src.shape
    d = L.GanTileGatherFDesc(_FLOAT[src.dtype], src.data_ptr(), src.numel(), wfull * c, col0, h, w, c, tile, overlap, t0, n,
                             ctx.dt if dtype is None else dtype, dst_view)
    L.check(ctx.lib.gan_tile_gather(C.byref(d), ctx.stream()), "tile_gather")


def blend_tiles(ctx, tiles_view, image, *, tile, overlap, t0, n, accumulate, dtype=None):
    """Tiles [t0, t0 + n) (a GanTensor of n x tile x tile, C channels) -> the dense fp32 `image` [h, w, C], weighted."""
    h, w, c = image.shape
    d = L.GanTileBlendDesc(ctx.dt if dtype is None else dtype, tiles_view, image.data_ptr(), h, w, c, tile, overlap, t0, n,
                           int(bool(accumulate)))
    L.check(ctx.lib.gan_tile_blend(C.byref(d), ctx.stream()), "tile_blend")


def cut_tiles(image, tile, overlap, col0=0, width=None):
    """What the two gathers cut, restated with slices: the tiles of columns [col0, col0 + width) of `image` ([H, Wfull, C], a
    tensor on any device or an array), row-major -> [nt, tile, tile, C] of the image's own type (no table, no cast)."""
    w = image.shape[1] - col0 if width is None else int(width)
    oys, oxs = tile_origins(image.shape[0], tile, overlap), tile_origins(w, tile, overlap)
    parts = [image[oy:oy + tile, col0 + ox:col0 + ox + tile] for oy in oys for ox in oxs]
    return torch.stack(parts) if isinstance(image, torch.Tensor) else np.stack(parts)


def infer_tiled(model, src, *, tile, overlap, col0=0, width=None, batch=None, fold=True):
    """`model` (a GeneratorModel) in inference mode over the whole image: -> fp32 device tensor [H, width, C].
    src: a device tensor [H, Wfull, C], either uint8 (normalised through the table by gan_tile_gather_u8) or float - fp32, or the
    model's storage type - holding normalised values already (gan_tile_gather: the fp32 output of another infer_tiled, say); the
    part used is the columns [col0, col0 + width) (width None: up to the right edge) - the left or right half of a pair without
    a copy.  The tiles run through the eval call of `batch` samples (None: all tiles of the image in one call), the last chunk
    through a call of its own size; the gather writes the call's typed input, the blend reads its typed output.  fold=False:
    model.fold() ran since the weights last changed."""
    ctx = model.net.ctx
    if not isinstance(src, torch.Tensor) or src.dim() != 3 or not src.is_contiguous() or src.device != torch.device(ctx.device):
        raise ValueError("infer_tiled: expected a contiguous [H, W, C] tensor on the model's device")
    if src.dtype == torch.uint8:
        gather = gather_tiles
    elif src.dtype == torch.float32 or (src.dtype in _FLOAT and _FLOAT[src.dtype] == ctx.dt):
        gather = gather_tiles_f
    else:
        raise ValueError(f"infer_tiled: a {src.dtype} source; expected uint8, float32 or the model's storage type")
    H, wfull, c = src.shape
    w = wfull - col0 if width is None else int(width)
    if c != model.net.channels or col0 < 0 or w < 1 or col0 + w > wfull:
        raise ValueError(f"infer_tiled: {c} channels, columns [{col0}, {col0 + w}) of a {wfull}-column image with a "
                         f"{model.net.channels}-channel generator")
    ny, nx = tile_grid(H, w, tile, overlap)
    nt = ny * nx
    chunk = nt if batch is None else max(1, min(int(batch), nt))
    if fold:
        model.fold()
    image = torch.empty((H, w, c), dtype=torch.float32, device=ctx.device)
    for t0 in range(0, nt, chunk):
        n = min(chunk, nt - t0)
        call = model.eval_call(n, tile)
        gather(ctx, src, call.xin.view(0, c, 0, n), h=H, w=w, tile=tile, overlap=overlap, t0=t0, n=n, col0=col0)
        call.infer(fold=False)
        blend_tiles(ctx, call.out_view(0, n), image, tile=tile, overlap=overlap, t0=t0, n=n, accumulate=t0 > 0)
    return image
