"""Reference of the dSSIM loss (include/gan_amd.h: gan_dssim) in torch on the CPU, written from the
definition and sharing no code with the kernel: display range u = 0.5 * x + 0.5, Gaussian window of 11 taps (sigma 1.5) applied as
ONE depthwise 11 x 11 conv2d with VALID padding, S = A1 A2 / (B1 B2) in the uncentred moments, loss = 1 - mean_i ssim_i, and the
gradient by torch.autograd.  dtype float64 is the reference; the same code in float32 is the yardstick of the gradient tests.
Inputs: NHWC arrays / tensors of raw values in [-1, 1], taken to `dtype` AS STORED."""
import numpy as np
import torch
import torch.nn.functional as F

C1, C2 = 1e-4, 9e-4


def window2d(dtype=torch.float64):
    k = torch.arange(11, dtype=torch.float64) - 5.0
    g = torch.exp(-k * k / (2.0 * 1.5 * 1.5))
    g = g / g.sum()
    return torch.outer(g, g).to(dtype)


def _nchw(x, dtype):
    x = torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x)
    return x.detach().cpu().to(dtype).permute(0, 3, 1, 2).contiguous()


def ssim_map(a, b):
    """S per (image, channel, map position) of two NCHW tensors of raw values."""
    c = a.shape[1]
    ua, ub = 0.5 * a + 0.5, 0.5 * b + 0.5
    win = window2d(a.dtype).expand(c, 1, 11, 11).contiguous()
    flt = lambda t: F.conv2d(t, win, groups=c)
    mx, my, sxy, sq = flt(ua), flt(ub), flt(ua * ub), flt(ua * ua + ub * ub)
    a1, b1 = 2 * mx * my + C1, mx * mx + my * my + C1
    a2, b2 = 2 * (sxy - mx * my) + C2, sq - mx * mx - my * my + C2
    return (a1 * a2) / (b1 * b2)


def loss_and_grad(a, b, dtype=torch.float64):
    """-> (loss: python float, dloss/da: NHWC tensor of `dtype`)"""
    at = _nchw(a, dtype).requires_grad_(True)
    bt = _nchw(b, dtype)
    loss = 1.0 - ssim_map(at, bt).mean(dim=(2, 3)).mean(dim=1).mean()
    loss.backward()
    return float(loss.detach()), at.grad.permute(0, 2, 3, 1).contiguous()


def loss(a, b, dtype=torch.float64):
    with torch.no_grad():
        return float(1.0 - ssim_map(_nchw(a, dtype), _nchw(b, dtype)).mean(dim=(2, 3)).mean(dim=1).mean())
