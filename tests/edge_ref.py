"""float64 numpy restatement of the Sobel edge term (include/gan_amd.h: gan_edge_l1), written from the formula:

    d = a - b;  ex(q) = (Sx * d)(q) / 8, ey(q) = (Sy * d)(q) / 8 at the valid positions 1 <= qy <= h-2, 1 <= qx <= w-2 (correlation,
    nothing padded);  M = (h-2)(w-2);  loss = sum (|ex| + |ey|) / (2 n c M);  dloss/da(p) = k(p) / (16 n c M) with
    k(p) = sum over the valid q, |q - p|_inf <= 1, of Sx(p - q) sgn(ex(q)) + Sy(p - q) sgn(ey(q)),  sgn(0) = 0.

Arrays are NHWC."""
import numpy as np

SX = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.float64)
SY = SX.T.copy()


def responses(a, b):
    """-> (ex, ey), each [n, h-2, w-2, c]: entry [.., i, j, ..] is the valid position q = (i + 1, j + 1)."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    n, h, w, c = d.shape
    ex = np.zeros((n, h - 2, w - 2, c))
    ey = np.zeros((n, h - 2, w - 2, c))
    for i in range(3):
        for j in range(3):
            win = d[:, i:i + h - 2, j:j + w - 2, :]
            ex += SX[i, j] * win
            ey += SY[i, j] * win
    return ex / 8.0, ey / 8.0


def abs_sum(a, b):
    """Sum of the absolute terms |ex| + |ey| (the loss's numerator)."""
    ex, ey = responses(a, b)
    return float(np.abs(ex).sum() + np.abs(ey).sum())


def loss(a, b):
    n, h, w, c = np.asarray(a).shape
    return abs_sum(a, b) / (2.0 * n * c * (h - 2) * (w - 2))


def k_map(a, b):
    """The integer map k(p), [n, h, w, c] int64: every valid position scatters its two signs onto its 3 x 3 pixels."""
    ex, ey = responses(a, b)
    n, h, w, c = np.asarray(a).shape
    sx, sy = np.sign(ex).astype(np.int64), np.sign(ey).astype(np.int64)
    k = np.zeros((n, h, w, c), dtype=np.int64)
    for i in range(3):          # pixel p = q + (i - 1, j - 1): d ex(q) / d d(p) = Sx[i, j]
        for j in range(3):
            k[:, i:i + h - 2, j:j + w - 2, :] += int(SX[i, j]) * sx + int(SY[i, j]) * sy
    return k


def loss_and_grad(a, b):
    n, h, w, c = np.asarray(a).shape
    return loss(a, b), k_map(a, b).astype(np.float64) / (16.0 * n * c * (h - 2) * (w - 2))


def min_response(a, b):
    """Per pixel p, the smallest |ex| or |ey| over the valid positions that contribute to k(p) (inf where none does)."""
    ex, ey = responses(a, b)
    n, h, w, c = np.asarray(a).shape
    m = np.minimum(np.abs(ex), np.abs(ey))
    out = np.full((n, h, w, c), np.inf)
    for i in range(3):
        for j in range(3):
            view = out[:, i:i + h - 2, j:j + w - 2, :]
            np.minimum(view, m, out=view)
    return out
