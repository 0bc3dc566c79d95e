"""Image preprocessing at read-in: the chain the reference runs offline with OpenCV in
create_training_imgs/curate_FLIR_data.py - contrast-limited adaptive histogram equalisation (cv2.createCLAHE(clipLimit=1.0,
tileGridSize=(15, 15))), a Gaussian blur of sigma 0.5 and a 3 x 3 sharpening filter - on decoded uint8 images, bytes in, bytes out.

`Preprocess.apply_host` is the vectorised numpy form (the host pipeline and prediction use it), `Preprocess.apply_device` runs the
same arithmetic over a device buffer through gan_preprocess_u8 (include/gan_amd.h); both produce the same bytes, and
tests/preprocess_ref.py restates them pixel by pixel.  A stage works on a REGION (a height x width window of an interleaved
image), reads nothing outside it (reflect-101 borders of the region itself) and treats every channel as its own plane: an RGB
image is equalised per channel, there is no colour-space conversion.  The order is fixed: clahe, blur, sharpen.  Parity with
OpenCV's own bytes is not pinned (there is no cv2 here to record from); the blur does not claim OpenCV's fixed-point taps."""
from __future__ import annotations

import ctypes
import math

import numpy as np

STAGES = ('clahe', 'blur', 'sharpen')
MAX_GRID, MAX_SIGMA = 32, 1.5


def parse_stages(text):
    """'sharpen, clahe' -> ('clahe', 'sharpen'): a comma-separated subset of STAGES in the fixed order; ValueError otherwise."""
    names = [n.strip() for n in str(text or '').split(',') if n.strip()]
    for n in names:
        if n not in STAGES:
            raise ValueError(f"unknown stage {n!r} (a comma-separated subset of {','.join(STAGES)})")
    if len(set(names)) != len(names):
        raise ValueError(f"a stage is named twice in {text!r}")
    return tuple(s for s in STAGES if s in names)


def blur_radius(sigma: float) -> int:
    return (int(round(6.0 * sigma + 1.0)) | 1) // 2         # (round(): half to even, as rint)


def blur_taps(sigma: float):
    """Integer taps q[-r .. r] that sum to 256: q_i = rint(256 w_i) off the centre, the centre takes the rest (float64)."""
    r = blur_radius(sigma)
    w = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(r + 1)]
    total = w[0] + 2.0 * sum(w[1:])
    q = [int(round(256.0 * (v / total))) for v in w]
    q[0] = 256 - 2 * sum(q[1:])
    return tuple(q[:0:-1]) + tuple(q)


def _f32(v):
    return float(np.float32(v))


class Preprocess:
    """stages: subset of STAGES (any order, or their comma-separated string); clip: CLAHE clip limit (0: none); grid: CLAHE tiles
    per side; sigma: blur.  clip and sigma are held as the values their float32 forms have, which is what the device entry point
    receives.  str(p) is canonical ('clahe,blur:clip=1.0,grid=15,sigma=0.5', '' for no stage) and Preprocess.parse reads it back."""

    def __init__(self, stages=(), clip=1.0, grid=15, sigma=0.5):
        self.stages = parse_stages(stages if isinstance(stages, str) else ','.join(stages))
        self.clip, self.grid, self.sigma = _f32(clip), int(grid), _f32(sigma)
        if int(grid) != grid or not 1 <= self.grid <= MAX_GRID:
            raise ValueError(f"clahe grid {grid} must be a whole number in 1 .. {MAX_GRID}")
        if not (math.isfinite(self.clip) and self.clip >= 0.0):
            raise ValueError(f"clahe clip {clip} must be finite and >= 0 (0: no clipping)")
        if not 0.0 < self.sigma <= MAX_SIGMA:
            raise ValueError(f"blur sigma {sigma} must be in (0, {MAX_SIGMA}]")

    @classmethod
    def parse(cls, text):
        stages, _, rest = str(text or '').partition(':')
        kw = {}
        for item in [i for i in rest.split(',') if i.strip()]:
            k, eq, v = item.partition('=')
            if not eq or k.strip() not in ('clip', 'grid', 'sigma'):
                raise ValueError(f"preprocess: cannot read {item!r} (clip=, grid=, sigma=)")
            kw[k.strip()] = int(v) if k.strip() == 'grid' else float(v)
        return cls(stages, **kw)

    def __str__(self):
        return f"{','.join(self.stages)}:clip={self.clip!r},grid={self.grid},sigma={self.sigma!r}" if self.stages else ''

    def __repr__(self):
        return f"Preprocess({str(self)!r})"

    def __bool__(self):
        return bool(self.stages)

    def __eq__(self, other):
        return isinstance(other, Preprocess) and str(self) == str(other)

    def __hash__(self):
        return hash(str(self))

    def check_region(self, height, width):
        """ValueError for a region a stage refuses (the device entry point's GAN_E_SHAPE)."""
        need = 1
        if 'clahe' in self.stages:
            need = max(need, self.grid)
        if 'blur' in self.stages:
            need = max(need, blur_radius(self.sigma) + 1)
        if 'sharpen' in self.stages:
            need = max(need, 2)
        if height < need or width < need:
            raise ValueError(f"preprocess {self}: a {height} x {width} region is smaller than {need} x {need}")

    # ---- host ------------------------------------------------------------------------------------------------------------------
    def apply_host(self, img_u8, regions=None):
        """-> a copy of the HWC (or HW) uint8 image with every region (y0, x0, height, width) - default: the whole image - run
        through the stages; everything outside the regions is the input's bytes."""
        img = np.array(img_u8, dtype=np.uint8, copy=True)
        if not self.stages:
            return img
        view = img[..., None] if img.ndim == 2 else img
        for y0, x0, h, w in ([(0, 0) + view.shape[:2]] if regions is None else regions):
            if y0 < 0 or x0 < 0 or h < 1 or w < 1 or y0 + h > view.shape[0] or x0 + w > view.shape[1]:
                raise ValueError(f"preprocess: region {(y0, x0, h, w)} lies outside the {view.shape[0]} x {view.shape[1]} image")
            self.check_region(h, w)
            for ch in range(view.shape[2]):
                plane = view[y0:y0 + h, x0:x0 + w, ch]
                for stage in self.stages:
                    plane = {'clahe': self._clahe, 'blur': self._blur, 'sharpen': self._sharpen}[stage](plane)
                view[y0:y0 + h, x0:x0 + w, ch] = plane
        return img

    def _clahe(self, p):
        h, w = p.shape
        g = self.grid
        th, tw = -(-h // g), -(-w // g)
        area = th * tw
        pad = np.pad(p, ((0, th * g - h), (0, tw * g - w)), mode='reflect')
        tiles = pad.reshape(g, th, g, tw).transpose(0, 2, 1, 3).reshape(g * g, area).astype(np.int64)
        hist = np.bincount((tiles + 256 * np.arange(g * g)[:, None]).ravel(), minlength=256 * g * g).reshape(g * g, 256)
        if self.clip > 0.0:
            limit = max(int(self.clip * area / 256), 1)
            clipped = np.maximum(hist - limit, 0).sum(axis=1)
            hist = np.minimum(hist, limit)
            batch = clipped // 256
            residual = clipped - 256 * batch
            hist = hist + batch[:, None]
            step = np.maximum(256 // np.maximum(residual, 1), 1)[:, None]
            i = np.arange(256)[None, :]
            hist = hist + ((i % step == 0) & (i // step < residual[:, None]))
        scale = np.float32(255.0 / area)
        lut = np.clip(np.rint(np.cumsum(hist, axis=1).astype(np.float32) * scale), 0, 255).astype(np.float32).reshape(g, g, 256)
        half, one = np.float32(0.5), np.float32(1.0)

        def axis(n, t):
            f = np.arange(n, dtype=np.float32) * (one / np.float32(t)) - half
            lo = np.floor(f)
            a = f - lo
            lo = lo.astype(np.int64)
            return np.maximum(lo, 0), np.minimum(lo + 1, g - 1), a, one - a
        ty1, ty2, ya, ya1 = (v[:, None] for v in axis(h, th))
        tx1, tx2, xa, xa1 = (v[None, :] for v in axis(w, tw))
        v = p.astype(np.int64)
        top = lut[ty1, tx1, v] * xa1 + lut[ty1, tx2, v] * xa
        bot = lut[ty2, tx1, v] * xa1 + lut[ty2, tx2, v] * xa
        out = np.rint(top * ya1 + bot * ya)
        assert out.dtype == np.float32
        return np.clip(out, 0, 255).astype(np.uint8)

    def _blur(self, p):
        q = blur_taps(self.sigma)
        r = len(q) // 2
        h, w = p.shape
        pad = np.pad(p.astype(np.int64), r, mode='reflect')
        t = sum(q[k] * pad[:, k:k + w] for k in range(2 * r + 1))
        u = sum(q[k] * t[k:k + h] for k in range(2 * r + 1))
        return ((u + 32768) >> 16).astype(np.uint8)

    def _sharpen(self, p):
        h, w = p.shape
        e = np.pad(p.astype(np.int64), 1, mode='reflect')
        out = 5 * e[1:-1, 1:-1] - e[:-2, 1:-1] - e[2:, 1:-1] - e[1:-1, :-2] - e[1:-1, 2:]
        return np.clip(out, 0, 255).astype(np.uint8)

    # ---- device ----------------------------------------------------------------------------------------------------------------
    def descriptor(self, channels, regions, src_ptr=None, src_bytes=0):
        """-> (GanPreprocessDesc, the ctypes region array it points to - keep it alive) for `regions` = (byte offset, row pitch in
        bytes, height, width) in a packed uint8 buffer; workspace not set."""
        from . import _lib as L
        arr = (L.GanPreRegion * max(len(regions), 1))()
        for s, (off, pitch, h, w) in zip(arr, regions):
            s.src_offset, s.pitch, s.height, s.width = int(off), int(pitch), int(h), int(w)
        bits = sum(b for n, b in zip(STAGES, (L.PRE_CLAHE, L.PRE_BLUR, L.PRE_SHARPEN)) if n in self.stages)
        d = L.GanPreprocessDesc(len(regions), int(channels), bits, src_ptr, int(src_bytes), self.clip, self.grid, self.sigma, None, 0,
                                ctypes.addressof(arr))
        return d, arr

    def apply_device(self, buffer, regions, stream=None, channels=1):
        """Enqueue the stages over `regions` = (byte offset, row pitch in bytes, height, width) of the 1-D uint8 device tensor
        `buffer`, in place, on `stream` (default: the current one).  No host synchronisation; the workspace is allocated here and
        handed back to the caching allocator, which keeps it for the stream until the launches are through."""
        import torch
        from . import _lib as L
        if not self.stages or not regions:
            return buffer
        assert buffer.dtype == torch.uint8 and buffer.dim() == 1 and buffer.is_contiguous() and buffer.is_cuda
        for _, _, h, w in regions:
            self.check_region(h, w)
        lib = L.load()
        d, arr = self.descriptor(channels, regions, buffer.data_ptr(), buffer.numel())
        need = lib.gan_preprocess_workspace_bytes(ctypes.byref(d))
        if need == 0:
            raise L.GanAmdError(f"preprocess {self}: the descriptor is refused (channels {channels}, {len(regions)} regions)")
        with torch.cuda.device(buffer.device):
            if stream is None:
                stream = torch.cuda.current_stream(buffer.device)
            with torch.cuda.stream(stream):
                ws = torch.empty(need, dtype=torch.uint8, device=buffer.device)
                d.workspace, d.workspace_bytes = ws.data_ptr(), need
                L.check(lib.gan_preprocess_u8(ctypes.byref(d), stream.cuda_stream), "preprocess_u8")
        return buffer
