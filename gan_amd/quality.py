"""Image-quality metrics on the device (include/gan_amd.h: gan_image_quality): SSIM as tf.image.ssim
defines it, PSNR, MAE and MSE between a prediction and its target, per image, on the display range 0.5 * x + 0.5.

`image_quality` enqueues the two launches on the current stream and returns the device tensor; `QualityMeter` keeps the rows of a
whole pass on the device and drains them once, as `run_epochs` does with the losses.  The reference has no such measurement: its
only SSIM compares the input with the target (pix2pix.py:182-184)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _lib as L
from .nets import Buf

KEYS = ('SSIM', 'PSNR', 'MAE', 'MSE')        # column order of gan_image_quality's `out`
_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}


def _operand(ctx, x, c=None):
    """-> (GanTensor, dtype code, object to keep alive).  x: a GanTensor view in the context's storage dtype, a nets.Buf (its first
    `c` channels), a dense NHWC tensor in fp32 / bf16 / fp16, or anything torch.as_tensor takes (then fp32 on the device)."""
    if isinstance(x, L.GanTensor):
        return x, ctx.dt, None
    if isinstance(x, Buf):
        return x.view(0, x.c if c is None else c), _DT[x.t.dtype], x
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    x = torch.as_tensor(x)
    if x.dtype not in _DT:
        x = x.float()
    x = x.to(ctx.device).contiguous()
    if x.dim() != 4:
        raise ValueError(f"image_quality: expected an NHWC batch, got shape {tuple(x.shape)}")
    n, h, w, ch = x.shape
    return L.GanTensor(x.data_ptr(), n, h, w, ch, ch), _DT[x.dtype], x


def image_quality(ctx, pred, target, out=None):
    """-> float32 device tensor [n, 4] = {SSIM, PSNR, MAE, MSE} per image (KEYS).  pred: typed Buf / GanTensor view (for instance
    the generator's 8-channel-padded output view: no unpack) or a dense tensor; target: dense tensor or array.  Enqueue-only on the
    current stream; the workspace is cached per shape on the context (calls of one shape must be stream-ordered)."""
    tb, dtb, keep_b = _operand(ctx, target)
    ta, dta, keep_a = _operand(ctx, pred, tb.c)
    n, h, w, c = tb.n, tb.h, tb.w, tb.c
    cache = ctx.__dict__.setdefault('_quality_ws', {})
    key = (n, h, w, c)
    if key not in cache:
        need = ctx.lib.gan_image_quality_workspace_bytes(n, h, w, c)
        cache[key] = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=ctx.device)
    ws = cache[key]
    if out is None:
        out = torch.empty((n, 4), dtype=torch.float32, device=ctx.device)
    d = L.GanQualityDesc(dta, dtb, ta, tb, out.data_ptr(), ws.data_ptr(), ws.numel() * 4)
    L.check(ctx.lib.gan_image_quality(C.byref(d), ctx.stream()), "image_quality")
    return out


def ms_ssim(ctx, pred, target, scales=5, power=None):
    """-> float32 device tensor [n]: the MS-SSIM of every image (include/gan_amd.h: gan_msssim as a metric - loss only, per_image;
    DESIGN.md section 24).  Operands as image_quality's; power: `scales` factors (default: tf.image.ssim_multiscale's first
    `scales`).  Enqueue-only on the current stream; the workspace is cached per shape on the context.  A shape the kernel
    refuses (a side below 11 * 2^(scales - 1)) raises ValueError."""
    tb, dtb, keep_b = _operand(ctx, target)
    ta, dta, keep_a = _operand(ctx, pred, tb.c)
    n, h, w, c = tb.n, tb.h, tb.w, tb.c
    pw = L.msssim_power(scales, power)
    cache = ctx.__dict__.setdefault('_msssim_ws', {})
    key = (n, h, w, c, scales)
    if key not in cache:
        need = ctx.lib.gan_msssim_workspace_bytes(n, h, w, c, scales)
        if not need:
            raise ValueError(f"ms_ssim: unsupported shape {(n, h, w, c)} for {scales} scales")
        cache[key] = torch.empty(need // 4 + 1, dtype=torch.float32, device=ctx.device)       # (+ 1: the loss word)
    ws = cache[key]
    out = torch.empty((n,), dtype=torch.float32, device=ctx.device)
    d = L.GanMsssimDesc(dta, dtb, ta, tb, 1.0, 0, ws.data_ptr() + 4 * (ws.numel() - 1), 0.0, L.F32, L.GanTensor(), ws.data_ptr(),
                        (ws.numel() - 1) * 4, None, scales, pw, out.data_ptr(), 0)
    L.check(ctx.lib.gan_msssim(C.byref(d), ctx.stream()), "msssim")
    return out


class QualityMeter:
    """Per-image rows of a pass, kept on the device: add() never synchronises, drain() makes the one transfer."""

    def __init__(self):
        self.rows = []

    def add(self, rows):
        self.rows.append(rows)

    def __len__(self):
        return sum(r.shape[0] for r in self.rows)

    def sums(self):
        """-> (device tensor [4]: column sums, number of images) without a sync; (None, 0) when nothing was added."""
        if not self.rows:
            return None, 0
        return torch.cat(self.rows).double().sum(dim=0), len(self)

    def drain(self, keys=KEYS):
        """-> {'SSIM': [...], 'PSNR': [...], 'MAE': [...], 'MSE': [...]} per image in the order added; empties the meter.
        keys: the names of the columns of the rows that were added (gan_amd.cycle_quality adds wider rows)."""
        rows, self.rows = self.rows, []
        host = torch.cat(rows).cpu().tolist() if rows else []
        return {k: [r[j] for r in host] for j, k in enumerate(keys)}


def _finite(v):
    return v if math.isfinite(v) else None


def summary(per_image):
    """{'per_image': ..., 'mean': ...} ready for strict JSON: a non-finite value (the PSNR of an exact match) becomes null."""
    mean = {k: (float(np.mean(np.asarray(v, np.float64))) if len(v) else float('nan')) for k, v in per_image.items()}
    return {'per_image': {k: [_finite(float(x)) for x in v] for k, v in per_image.items()},
            'mean': {k: _finite(v) for k, v in mean.items()}}
