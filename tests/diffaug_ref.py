"""float64 restatement of the differentiable augmentation (include/gan_amd.h: GanDiffAugParams, gan_diffaug_draw,
gan_diffaug_apply) on the CPU, sharing no code with the kernels: the draws from the header's bit layout in
Python integers, the forward map from index gathers (so that torch autograd yields its backward), and the closed form of the
transpose in numpy.  The arbiter of tests/test_cpu_diffaug.py (which pins it), test_gpu_diffaug.py and test_gpu_diffaug_step.py."""
import numpy as np
import torch

M64 = (1 << 64) - 1
POLICIES = ('translation', 'cutout', 'brightness', 'saturation')
NEUTRAL = dict(tx=0, ty=0, cut_x0=0, cut_y0=0, cut_w=0, cut_h=0, brightness=0.0, saturation=1.0)


def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _cut_axis(bits32, size):
    cs = size // 2
    n = size + (1 - cs % 2)
    start = ((bits32 * n) >> 32) - cs // 2
    lo, hi = max(start, 0), min(start + cs, size)
    return lo, hi - lo


def draw(seed, launches, stream_id, n, h, w, policies):
    """The n records launch number `launches` (0-based value of the counter when the launch reads it) writes."""
    key = mix64((seed ^ ((launches & 0xffffffff) << 32) ^ stream_id) & M64)
    out = []
    for i in range(n):
        hk = [mix64(key ^ (4 * i + k)) for k in range(4)]
        p = dict(NEUTRAL)
        if 'translation' in policies:
            Tx, Ty = (w + 4) // 8, (h + 4) // 8
            p['tx'] = (((hk[0] & 0xffffffff) * (2 * Tx + 1)) >> 32) - Tx
            p['ty'] = (((hk[0] >> 32) * (2 * Ty + 1)) >> 32) - Ty
        if 'cutout' in policies:
            x0, cw = _cut_axis(hk[1] & 0xffffffff, w)
            y0, ch = _cut_axis(hk[1] >> 32, h)
            if cw > 0 and ch > 0:
                p.update(cut_x0=x0, cut_y0=y0, cut_w=cw, cut_h=ch)
        if 'brightness' in policies:
            p['brightness'] = (hk[2] >> 40) * 2.0 ** -24 - 0.5
        if 'saturation' in policies:
            p['saturation'] = (hk[3] >> 40) * 2.0 ** -23
        out.append(p)
    return out


def table(params):
    """list of records -> the int32 [n, 8] image of the 32-byte device records (floats as their fp32 bits)."""
    t = np.zeros((len(params), 8), dtype=np.int32)
    for i, p in enumerate(params):
        t[i, :6] = [p['tx'], p['ty'], p['cut_x0'], p['cut_y0'], p['cut_w'], p['cut_h']]
        t[i, 6:] = np.array([p['brightness'], p['saturation']], dtype=np.float32).view(np.int32)
    return t


def records(tab):
    """the inverse of table()."""
    tab = np.asarray(tab, dtype=np.int32)
    f = tab[:, 6:].copy().view(np.float32)
    keys = ('tx', 'ty', 'cut_x0', 'cut_y0', 'cut_w', 'cut_h')
    return [dict(zip(keys, (int(v) for v in tab[i, :6])), brightness=float(f[i, 0]), saturation=float(f[i, 1])) for i in range(len(tab))]


def _cut_mask(p, h, w):
    """[h, w] bool: the cut rectangle in output coordinates."""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
    if p['cut_w'] <= 0:
        return np.zeros((h, w), dtype=bool)
    return (xx >= p['cut_x0']) & (xx < p['cut_x0'] + p['cut_w']) & (yy >= p['cut_y0']) & (yy < p['cut_y0'] + p['cut_h'])


def forward(x, params, group_c, sample0=0):
    """x: float64 torch [n, h, w, c] (may require grad) -> y, same shape: colour, translation with zero fill, cutout."""
    n, h, w, c = x.shape
    assert c % group_c == 0
    out = []
    for b in range(n):
        p = params[sample0 + b]
        xb = x[b].reshape(h, w, c // group_c, group_c)
        m = xb.mean(dim=3, keepdim=True)
        col = ((xb - m) * p['saturation'] + m + p['brightness']).reshape(h, w, c)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        qy, qx = yy - p['ty'], xx - p['tx']
        live = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w) & ~_cut_mask(p, h, w)
        idx = torch.from_numpy((np.clip(qy, 0, h - 1) * w + np.clip(qx, 0, w - 1)).reshape(-1))
        g = col.reshape(h * w, c).index_select(0, idx).reshape(h, w, c)
        out.append(g * torch.from_numpy(live.astype(np.float64))[:, :, None])
    return torch.stack(out)


def transpose(dy, params, group_c, sample0=0):
    """Closed form of the backward map: dx(q) = live(q + t) ? s dy(q + t) + (1 - s) mean_group(dy(q + t)) : 0.  numpy float64."""
    dy = np.asarray(dy, dtype=np.float64)
    n, h, w, c = dy.shape
    dx = np.zeros_like(dy)
    for b in range(n):
        p = params[sample0 + b]
        cut = _cut_mask(p, h, w)
        s = p['saturation']
        for qy in range(h):
            for qx in range(w):
                ry, rx = qy + p['ty'], qx + p['tx']
                if not (0 <= ry < h and 0 <= rx < w) or cut[ry, rx]:
                    continue
                g = dy[b, ry, rx].reshape(c // group_c, group_c)
                dx[b, qy, qx] = (s * g + (1 - s) * g.mean(axis=1, keepdims=True)).reshape(c)
    return dx


def autograd_transpose(dy, params, group_c, sample0=0):
    """The same through torch autograd on forward()."""
    dy = torch.as_tensor(np.asarray(dy, dtype=np.float64))
    x = torch.zeros_like(dy, requires_grad=True)
    forward(x, params, group_c, sample0).backward(dy)
    return x.grad.numpy()


def forward_terms(x, params, group_c, sample0=0):
    """|largest term| of the forward arithmetic per output element (x, m, s (x - m), brightness at the source pixel; 0 where the
    output is the fill): the magnitude the fp32 gate of the GPU test is taken at.  numpy [n, h, w, c]."""
    x = np.asarray(x, dtype=np.float64)
    n, h, w, c = x.shape
    big = np.zeros_like(x)
    for b in range(n):
        p = params[sample0 + b]
        xb = x[b].reshape(h, w, c // group_c, group_c)
        m = xb.mean(axis=3, keepdims=True)
        t = np.maximum.reduce([np.abs(xb).max(axis=3, keepdims=True) + 0 * xb, np.abs(m) + 0 * xb, np.abs(p['saturation'] * (xb - m)),
                               np.full_like(xb, abs(p['brightness']))]).reshape(h, w, c)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        qy, qx = yy - p['ty'], xx - p['tx']
        live = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w) & ~_cut_mask(p, h, w)
        big[b] = t[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)] * live[:, :, None]
    return big


def transpose_terms(dy, params, group_c, sample0=0):
    """The same for the backward arithmetic: max(|dy| of the group, |s dy|, |(1 - s) mean|) at the pixel read."""
    dy = np.asarray(dy, dtype=np.float64)
    n, h, w, c = dy.shape
    big = np.zeros_like(dy)
    for b in range(n):
        p = params[sample0 + b]
        s = p['saturation']
        gb = dy[b].reshape(h, w, c // group_c, group_c)
        m = gb.mean(axis=3, keepdims=True)
        t = np.maximum.reduce([np.abs(gb).max(axis=3, keepdims=True) + 0 * gb, np.abs(s * gb), np.abs((1 - s) * m) + 0 * gb]).reshape(h, w, c)
        cut = _cut_mask(p, h, w)
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing='ij')
        ry, rx = yy + p['ty'], xx + p['tx']
        inside = (ry >= 0) & (ry < h) & (rx >= 0) & (rx < w)
        ryc, rxc = np.clip(ry, 0, h - 1), np.clip(rx, 0, w - 1)
        live = inside & ~cut[ryc, rxc]
        big[b] = t[ryc, rxc] * live[:, :, None]
    return big


MANTISSA = {'f32': 23, 'bf16': 7, 'f16': 10}
MIN_EXP = {'f32': -126, 'bf16': -126, 'f16': -14}       # exponent of the smallest normal number


def ulp(v, dtype):
    """One unit in the last place of `dtype` at the magnitude of v (elementwise; the subnormal spacing below the normal range)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** MIN_EXP[dtype])))
    return 2.0 ** (np.maximum(e, MIN_EXP[dtype]) - MANTISSA[dtype])
