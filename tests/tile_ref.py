"""fp64 numpy reference of tiled inference, written from the definition and not from the kernels.

Per axis of length L, tile size S, overlap V, stride T = S - V: n = 1 if L == S else ceil((L - S) / T) + 1 tiles, tile k at
min(k T, L - S).  Weight of the offset i inside a tile: hat(i) = min(i + 1, S - i); a pixel's weight for a tile is its hat over the
sum of the hats of all tiles that cover it, per axis, and the two axes multiply.  Tiles are numbered row-major."""
import math

import numpy as np


def origins(L, S, V):
    assert S % 8 == 0 and 16 <= S <= 1024 and 0 <= V <= S // 2 and S <= L <= 4096, (L, S, V)
    T = S - V
    n = 1 if L == S else math.ceil((L - S) / T) + 1
    return [min(k * T, L - S) for k in range(n)]


def grid(h, w, S, V):
    return len(origins(h, S, V)), len(origins(w, S, V))


def axis_weights(L, S, V):
    """-> float64 [n, L]: weight of tile k at coordinate p (0 where the tile does not cover p); every column sums to 1."""
    org = origins(L, S, V)
    hat = np.zeros((len(org), L))
    i = np.arange(S)
    for k, o in enumerate(org):
        hat[k, o:o + S] = np.minimum(i + 1, S - i)
    return hat / hat.sum(axis=0, keepdims=True)


def cover_counts(L, S, V):
    return (axis_weights(L, S, V) > 0).sum(axis=0)


def cut(image, S, V):
    """image [h, w, c] -> [nt, S, S, c]: the tiles, row-major."""
    h, w = image.shape[:2]
    return np.stack([image[oy:oy + S, ox:ox + S] for oy in origins(h, S, V) for ox in origins(w, S, V)])


def blend(tiles, h, w, S, V, t0=0, n=None, start=None):
    """tiles [n, S, S, c] = tiles t0 .. t0 + n - 1 of the grid -> float64 [h, w, c]: start (zeros by default) plus the weighted
    tiles.  The weights are those of the whole grid, whichever tiles are present."""
    tiles = np.asarray(tiles, np.float64)
    oys, oxs = origins(h, S, V), origins(w, S, V)
    wy, wx = axis_weights(h, S, V), axis_weights(w, S, V)
    n = len(oys) * len(oxs) - t0 if n is None else n
    out = np.zeros((h, w, tiles.shape[-1])) if start is None else np.array(start, np.float64)
    for t in range(t0, t0 + n):
        ky, kx = divmod(t, len(oxs))
        oy, ox = oys[ky], oxs[kx]
        wgt = wy[ky, oy:oy + S, None] * wx[kx, None, ox:ox + S]
        out[oy:oy + S, ox:ox + S] += wgt[..., None] * tiles[t - t0]
    return out
