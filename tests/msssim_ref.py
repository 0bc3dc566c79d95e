"""Reference of the MS-SSIM loss (include/gan_amd.h: gan_msssim) in torch on the CPU, written from the
definition and sharing no code with the kernel: display range u = 0.5 * x + 0.5, Gaussian window of 11 taps (sigma 1.5) applied as
ONE depthwise 11 x 11 conv2d with VALID padding, lum and cs in the uncentred moments, the pyramid by indexing (2 x 2 mean with the
last row / column repeated where a side is odd), MS = prod max(CS_j, 0)^w_j * max(S_{M-1}, 0)^w_{M-1} per image and channel, the
score of an image the channel mean, loss = 1 - mean over the images, and the gradient by torch.autograd (the clamp has gradient 0,
and a clamped factor makes the whole product 0).  dtype float64 is the reference; the same code in float32 is the yardstick of the
gradient tests.  Inputs: NHWC arrays / tensors of raw values in [-1, 1], taken to `dtype` AS STORED."""
import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 1e-4, 9e-4
POWER = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)          # tf.image.ssim_multiscale


def shape_ok(h, w, scales):
    """The kernel's shape rule restated: 1 .. 5 scales, sides up to 4096 and at least 11 * 2^(scales - 1)."""
    return 1 <= scales <= 5 and min(h, w) >= 11 * 2 ** (scales - 1) and max(h, w) <= 4096


def window2d(dtype=torch.float64):
    k = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.exp(-k * k / (2.0 * 1.5 * 1.5))
    g = g / g.sum()
    return torch.outer(g, g).to(dtype)


def _nchw(x, dtype):
    x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return x.detach().cpu().to(dtype).permute(0, 3, 1, 2).contiguous()


def pool(x):
    """NCHW -> the next level: rows / columns (2i, min(2i + 1, last)), mean of the four taps."""
    h, w = x.shape[2], x.shape[3]
    r0 = torch.arange(0, h, 2)
    r1 = torch.clamp(r0 + 1, max=h - 1)
    c0 = torch.arange(0, w, 2)
    c1 = torch.clamp(c0 + 1, max=w - 1)
    top, bot = x[:, :, r0], x[:, :, r1]
    return 0.25 * ((top[:, :, :, c0] + top[:, :, :, c1]) + (bot[:, :, :, c0] + bot[:, :, :, c1]))


def level_terms(a, b):
    """(mean cs, mean lum * cs) per (image, channel) of two NCHW tensors of raw values."""
    c = a.shape[1]
    ua, ub = 0.5 * a + 0.5, 0.5 * b + 0.5
    win = window2d(a.dtype).expand(c, 1, 11, 11).contiguous()
    flt = lambda t: F.conv2d(t, win, groups=c)
    mx, my, sxy, sq = flt(ua), flt(ub), flt(ua * ub), flt(ua * ua + ub * ub)
    lum = (2 * mx * my + C1) / (mx * mx + my * my + C1)
    cs = (2 * (sxy - mx * my) + C2) / (sq - mx * mx - my * my + C2)
    return cs.mean(dim=(2, 3)), (lum * cs).mean(dim=(2, 3))


def factors(a, b, scales):
    """-> list of `scales` tensors [n, c]: CS_0 .. CS_{M-2}, S_{M-1} (unclamped)."""
    out = []
    for j in range(scales):
        cs, s = level_terms(a, b)
        out.append(s if j == scales - 1 else cs)
        if j + 1 < scales:
            a, b = pool(a), pool(b)
    return out


def scores(a, b, scales=5, power=None):
    """per-image MS-SSIM [n] of two NCHW tensors (differentiable)"""
    power = POWER[:scales] if power is None else power
    assert len(power) == scales
    ms = None
    for f, w in zip(factors(a, b, scales), power):
        pos = f > 0                  # max(f, 0)^w with the clamped region's gradient 0 by definition (no 0 * inf from pow at 0)
        t = torch.where(pos, torch.where(pos, f, torch.ones_like(f)) ** w, torch.full_like(f, 1.0 if w == 0 else 0.0))
        ms = t if ms is None else ms * t
    return ms.mean(dim=1)


def loss_and_grad(a, b, scales=5, power=None, dtype=torch.float64):
    """-> (loss: python float, dloss/da: NHWC tensor of `dtype`, per-image scores: numpy [n])"""
    at = _nchw(a, dtype).requires_grad_(True)
    bt = _nchw(b, dtype)
    sc = scores(at, bt, scales, power)
    loss = 1.0 - sc.mean()
    loss.backward()
    return float(loss.detach()), at.grad.permute(0, 2, 3, 1).contiguous(), sc.detach().double().numpy()


def loss(a, b, scales=5, power=None, dtype=torch.float64):
    with torch.no_grad():
        return float(1.0 - scores(_nchw(a, dtype), _nchw(b, dtype), scales, power).mean())


def min_factor(a, b, scales, dtype=torch.float64):
    """the smallest CS_j / S_{M-1} over images and channels: the premise of the GPU tests' loss gate"""
    with torch.no_grad():
        return float(min(f.min() for f in factors(_nchw(a, dtype), _nchw(b, dtype), scales)))
