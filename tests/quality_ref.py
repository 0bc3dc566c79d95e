"""fp64 numpy reference of the image-quality metrics (include/gan_amd.h: gan_image_quality), written from
the definition line by line: display range u = 0.5 * x + 0.5, max_val = 1, SSIM as
tf.image.ssim(u_a, u_b, max_val=1, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03), PSNR as tf.image.psnr, MAE, MSE.
Inputs: NHWC arrays of raw values in [-1, 1] (any float dtype: they are taken to float64 as stored)."""
import numpy as np

FILTER_SIZE, FILTER_SIGMA, K1, K2, MAX_VAL = 11, 1.5, 0.01, 0.03, 1.0
C1, C2 = (K1 * MAX_VAL) ** 2, (K2 * MAX_VAL) ** 2


def window():
    k = np.arange(FILTER_SIZE, dtype=np.float64)
    g = np.exp(-(k - (FILTER_SIZE - 1) / 2) ** 2 / (2 * FILTER_SIGMA ** 2))
    return g / g.sum()


def _filter(u):
    """Separable Gaussian, VALID padding, over axes 1 and 2 of an NHWC array."""
    g = window()
    n, h, w, c = u.shape
    rows = sum(g[k] * u[:, k:k + h - FILTER_SIZE + 1] for k in range(FILTER_SIZE))
    return sum(g[k] * rows[:, :, k:k + w - FILTER_SIZE + 1] for k in range(FILTER_SIZE))


def display(x):
    return 0.5 * np.asarray(x, dtype=np.float64) + 0.5


def ssim(a, b):
    """-> [n] float64"""
    ua, ub = display(a), display(b)
    mx, my = _filter(ua), _filter(ub)
    lum = (2 * mx * my + C1) / (mx ** 2 + my ** 2 + C1)
    # (mx^2 + my^2 is subtracted as one term: with a == b numerator and denominator are then the same roundings and SSIM is exactly 1)
    cs = (2 * _filter(ua * ub) - 2 * mx * my + C2) / (_filter(ua ** 2 + ub ** 2) - (mx ** 2 + my ** 2) + C2)
    return (lum * cs).mean(axis=(1, 2)).mean(axis=-1)


def mae(a, b):
    return np.abs(display(a) - display(b)).mean(axis=(1, 2, 3))


def mse(a, b):
    return ((display(a) - display(b)) ** 2).mean(axis=(1, 2, 3))


def psnr(a, b):
    with np.errstate(divide='ignore'):
        return -10.0 * np.log10(mse(a, b))


def quality(a, b):
    """-> [n, 4] float64 rows {ssim, psnr, mae, mse}: the layout of gan_image_quality's `out`."""
    return np.stack([ssim(a, b), psnr(a, b), mae(a, b), mse(a, b)], axis=1)
