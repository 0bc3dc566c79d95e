"""Scalar restatement of the preprocessing arithmetic, pixel by pixel and bin by bin in plain Python loops,
with np.float32 scalars for the CLAHE blend.  Independent of gan_amd/preprocess.py: nothing is imported from the package."""
import math

import numpy as np


def reflect(i, n):
    """reflect-101 (gfedcb|abcdefgh|gfedcba) of an index into 0 .. n - 1"""
    if i < 0:
        i = -i
    if i >= n:
        i = 2 * n - 2 - i
    assert 0 <= i < n
    return i


def clahe_luts(p, clip, grid):
    """-> (luts[ty][tx] = 256 ints, tw, th) of the plane p (list of rows)"""
    h, w = len(p), len(p[0])
    assert h >= grid and w >= grid
    tw, th = (w + grid - 1) // grid, (h + grid - 1) // grid
    area = tw * th
    scale = np.float32(255 / area)
    luts = []
    for ty in range(grid):
        row = []
        for tx in range(grid):
            hist = [0] * 256
            for y in range(ty * th, (ty + 1) * th):
                for x in range(tx * tw, (tx + 1) * tw):
                    hist[int(p[reflect(y, h)][reflect(x, w)])] += 1
            if clip > 0:
                limit = max(int(clip * area / 256), 1)
                clipped = 0
                for i in range(256):
                    if hist[i] > limit:
                        clipped += hist[i] - limit
                        hist[i] = limit
                batch = clipped // 256
                residual = clipped - 256 * batch
                for i in range(256):
                    hist[i] += batch
                if residual:
                    step = max(256 // residual, 1)
                    for i in range(256):
                        if i % step == 0 and i // step < residual:
                            hist[i] += 1
            lut, total = [], 0
            for i in range(256):
                total += hist[i]
                v = float(np.rint(np.float32(total) * scale))
                lut.append(int(min(max(v, 0.0), 255.0)))
            assert total == area
            row.append(lut)
        luts.append(row)
    return luts, tw, th


def clahe(p, clip, grid):
    h, w = len(p), len(p[0])
    L, tw, th = clahe_luts(p, clip, grid)
    f = np.float32
    inv_tw, inv_th = f(1) / f(tw), f(1) / f(th)
    out = [[0] * w for _ in range(h)]
    for y in range(h):
        tyf = f(y) * inv_th - f(0.5)
        t = math.floor(tyf)
        ya = tyf - f(t)
        ya1 = f(1) - ya
        ty1, ty2 = max(t, 0), min(t + 1, grid - 1)
        for x in range(w):
            txf = f(x) * inv_tw - f(0.5)
            s = math.floor(txf)
            xa = txf - f(s)
            xa1 = f(1) - xa
            tx1, tx2 = max(s, 0), min(s + 1, grid - 1)
            v = int(p[y][x])
            top = f(L[ty1][tx1][v]) * xa1 + f(L[ty1][tx2][v]) * xa
            bot = f(L[ty2][tx1][v]) * xa1 + f(L[ty2][tx2][v]) * xa
            res = top * ya1 + bot * ya
            assert type(res) is np.float32
            out[y][x] = int(min(max(float(np.rint(res)), 0.0), 255.0))
    return out


def blur_taps(sigma):
    r = (int(np.rint(6 * sigma + 1)) | 1) // 2
    assert 0 < sigma <= 1.5 and r <= 5
    w = {i: math.exp(-i * i / (2 * sigma * sigma)) for i in range(-r, r + 1)}
    total = sum(w.values())
    q = {i: int(np.rint(256 * w[i] / total)) for i in w if i != 0}
    q[0] = 256 - sum(q.values())
    return [q[i] for i in range(-r, r + 1)]


def blur(p, sigma):
    h, w = len(p), len(p[0])
    q = blur_taps(sigma)
    r = len(q) // 2
    assert h >= r + 1 and w >= r + 1
    t = [[sum(q[i + r] * int(p[y][reflect(x + i, w)]) for i in range(-r, r + 1)) for x in range(w)] for y in range(h)]
    assert max(max(row) for row in t) < 65536
    return [[(sum(q[j + r] * t[reflect(y + j, h)][x] for j in range(-r, r + 1)) + 32768) >> 16 for x in range(w)] for y in range(h)]


def sharpen(p):
    h, w = len(p), len(p[0])
    g = lambda y, x: int(p[reflect(y, h)][reflect(x, w)])
    return [[min(max(5 * g(y, x) - g(y - 1, x) - g(y + 1, x) - g(y, x - 1) - g(y, x + 1), 0), 255) for x in range(w)] for y in range(h)]


def apply(img, regions, stages, clip=1.0, grid=15, sigma=0.5):
    """img: HWC uint8 array; regions: (y0, x0, height, width); stages: subset of clahe / blur / sharpen, run in that order."""
    out = np.array(img, dtype=np.uint8, copy=True)
    for y0, x0, h, w in regions:
        for ch in range(out.shape[2]):
            p = [[int(v) for v in row] for row in out[y0:y0 + h, x0:x0 + w, ch]]
            if 'clahe' in stages:
                p = clahe(p, clip, grid)
            if 'blur' in stages:
                p = blur(p, sigma)
            if 'sharpen' in stages:
                p = sharpen(p)
            out[y0:y0 + h, x0:x0 + w, ch] = np.array(p, dtype=np.uint8)
    return out
