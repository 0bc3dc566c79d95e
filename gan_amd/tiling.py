"""Prediction at the source resolution (include/gan_amd.h: gan_tile_grid / gan_tile_gather_u8 / gan_tile_blend; DESIGN.md section
13): an image larger than the network's input is cut into overlapping tiles on the device, the tiles go through the inference call
as one batch, and the outputs are blended back with hat weights - no fp32 staging tensor, no host round trip.

`tile_origins` / `tile_grid` restate the geometry in pure Python (the same rules as the C side; tests compare the two).  The
reference has no such path: it resizes every image to img_size x img_size before it predicts (pix2pix.py:43-52)."""
from __future__ import annotations

import ctypes as C

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


def blend_tiles(ctx, tiles_view, image, *, tile, overlap, t0, n, accumulate, dtype=None):
    """Tiles [t0, t0 + n) (a GanTensor of n x tile x tile, C channels) -> the dense fp32 `image` [h, w, C], weighted."""
    h, w, c = image.shape
    d = L.GanTileBlendDesc(ctx.dt if dtype is None else dtype, tiles_view, image.data_ptr(), h, w, c, tile, overlap, t0, n,
                           int(bool(accumulate)))
    L.check(ctx.lib.gan_tile_blend(C.byref(d), ctx.stream()), "tile_blend")


def infer_tiled(model, src_u8, *, tile, overlap, col0=0, width=None, batch=None, fold=True):
    """`model` (a GeneratorModel) in inference mode over the whole image: -> fp32 device tensor [H, width, C].
    src_u8: uint8 device tensor [H, Wfull, C]; the part used is the columns [col0, col0 + width) (width None: up to the right
    edge) - the left or right half of a pair without a copy.  The tiles run through the eval call of `batch` samples (None: all
    tiles of the image in one call), the last chunk through a call of its own size; the gather writes the call's typed input,
    the blend reads its typed output.  fold=False: model.fold() ran since the weights last changed."""
    ctx = model.net.ctx
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 3 or not src_u8.is_contiguous() or src_u8.device != torch.device(ctx.device):
        raise ValueError("infer_tiled: expected a contiguous uint8 [H, W, C] tensor on the model's device")
    H, wfull, c = src_u8.shape
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
        gather_tiles(ctx, src_u8, call.xin.view(0, c, 0, n), h=H, w=w, tile=tile, overlap=overlap, t0=t0, n=n, col0=col0)
        call.infer(fold=False)
        blend_tiles(ctx, call.out_view(0, n), image, tile=tile, overlap=overlap, t0=t0, n=n, accumulate=t0 > 0)
    return image
