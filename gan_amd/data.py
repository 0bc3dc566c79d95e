"""Host-side input pipeline: the reference's tf.data / tf.image steps restated with
PIL + numpy — decode, left/right split, nearest-neighbour resize, random jitter, normalise, batch
(base_gan.py:26-61, pix2pix.py:34-165, cycle_gan.py:40-152).  CPU I/O, not part of the accelerated path; a
background thread decodes ahead (CPU only), the consuming thread pins and uploads.  `--data-cache device` replaces everything
after the decode: DeviceDataset keeps the uint8 images in HBM, DeviceBatches builds the same batches with gan_augment_u8."""
from __future__ import annotations

import contextlib
import ctypes
import os
import queue
import random
import threading

import numpy as np


def decode(image_file: str, channels: int) -> np.ndarray:
    """The decode of `load`: PNG/JPEG -> `channels` channels, uint8 HWC."""
    from PIL import Image
    with Image.open(image_file) as im:
        a = np.asarray(im.convert('L' if channels == 1 else 'RGB'), dtype=np.uint8)
    return a[..., None] if a.ndim == 2 else a


def load(image_file: str, channels: int) -> np.ndarray:
    """base_gan.py:26-44: decode PNG/JPEG to `channels` channels, float32 HWC in [0,255]."""
    return decode(image_file, channels).astype(np.float32)


def nearest_index(n_in: int, n_out: int) -> np.ndarray:
    """Source index of every output row / column of `resize_nearest`: floor((dst + 0.5) * in / out) in float64 (NOT the integer
    form ((2 dst + 1) in) // (2 out): the two differ for some sizes, and the device path follows this one)."""
    return np.minimum(np.floor((np.arange(n_out) + 0.5) * (n_in / n_out)).astype(np.int64), n_in - 1)


def resize_nearest(image: np.ndarray, height: int, width: int) -> np.ndarray:
    """tf.image.resize(method=NEAREST_NEIGHBOR) (base_gan.py:46-54): half-pixel centres,
    src = floor((dst + 0.5) * in / out)."""
    h, w = image.shape[:2]
    return image[nearest_index(h, height)][:, nearest_index(w, width)]


def normalize(image: np.ndarray) -> np.ndarray:
    """base_gan.py:56-61"""
    return (image / np.float32(127.5)) - np.float32(1)


def split_img(image: np.ndarray, input_img_orient: str = 'left'):
    """pix2pix.py:34-54: split a side-by-side pair at w // 2."""
    w = image.shape[1] // 2
    if input_img_orient == 'left':
        return image[:, :w, :], image[:, w:, :]
    return image[:, w:, :], image[:, :w, :]


def draw_jitter(rng):
    """The random draws of one example's jitter, in the order the host pipeline has always made them:
    -> (crop y, crop x, mirror)."""
    y, x = rng.integers(0, 31), rng.integers(0, 31)
    return int(y), int(x), bool(rng.random() > 0.5)


def random_jitter_pair(a, b, size, rng):
    """pix2pix.py:70-87: resize to size+30, joint random crop, joint random mirror."""
    a = resize_nearest(a, size + 30, size + 30)
    b = resize_nearest(b, size + 30, size + 30)
    y, x, flip = draw_jitter(rng)
    a, b = a[y:y + size, x:x + size], b[y:y + size, x:x + size]
    if flip:
        a, b = a[:, ::-1], b[:, ::-1]
    return a, b


def random_jitter_single(a, size, rng):
    """cycle_gan.py:58-72: same for one unpaired image."""
    a = resize_nearest(a, size + 30, size + 30)
    y, x, flip = draw_jitter(rng)
    a = a[y:y + size, x:x + size]
    if flip:
        a = a[:, ::-1]
    return a


def list_images(path):
    return sorted(i for i in os.listdir(path) if 'png' in i or 'jpg' in i)


def pix2pix_split(contents, seed, test_img, validation_size):
    """Seeded train/val/test split exactly as pix2pix.py:136-147."""
    random.seed(seed)
    test = random.sample(contents, test_img)
    val_obs = int(np.ceil((len(contents) - test_img) * validation_size))
    val = random.sample([i for i in contents if i not in test], val_obs)
    train = [i for i in contents if i not in test and i not in val]
    train = random.sample(train, len(train))
    return train, val, test


class Batches:
    """Re-iterable batched dataset.  `make_example(path) -> tuple of HWC float32 arrays`; batches are tuples of
    NHWC float32 torch tensors on `device`, the last partial batch kept (no drop_remainder, pix2pix.py:163)."""

    def __init__(self, files, make_example, batch_size, device=None, shuffle_seed=None, prefetch=2):
        self.files, self.make_example, self.bs = list(files), make_example, batch_size
        self.device, self.shuffle_seed, self.prefetch = device, shuffle_seed, prefetch
        self.epoch = 0

    def __len__(self):
        return (len(self.files) + self.bs - 1) // self.bs

    def _produce(self, files, q, stop):
        """Worker thread: decode + augment + stack on the CPU only.  It never touches the GPU (a pin_memory() or an upload
        from here could land inside the main thread's hipGraph capture and invalidate it); errors travel to the consumer."""
        import torch
        try:
            for i in range(0, len(files), self.bs):
                ex = [self.make_example(f) for f in files[i:i + self.bs]]
                item = tuple(torch.from_numpy(np.ascontiguousarray(np.stack([e[k] for e in ex]))) for k in range(len(ex[0])))
                while not stop.is_set():
                    try:
                        q.put(item, timeout=0.1)
                        break
                    except queue.Full:
                        continue
                if stop.is_set():
                    return
            item = None
        except BaseException as e:          # corrupt image, bad path ...: re-raised by __iter__
            item = e
        while not stop.is_set():
            try:
                q.put(item, timeout=0.1)
                return
            except queue.Full:
                continue

    def __iter__(self):
        files = self.files
        if self.shuffle_seed is not None:
            r = random.Random(self.shuffle_seed + self.epoch)
            files = r.sample(files, len(files))
        self.epoch += 1
        q, stop = queue.Queue(maxsize=self.prefetch), threading.Event()
        th = threading.Thread(target=self._produce, args=(files, q, stop), daemon=True)
        th.start()
        cuda = self.device is not None and str(self.device).startswith('cuda')
        try:
            while True:
                b = q.get()
                if b is None:
                    return
                if isinstance(b, BaseException):
                    raise b
                if self.device is not None:      # upload in the consumer (the thread that owns the stream / any capture)
                    b = tuple((t.pin_memory() if cuda else t).to(self.device, non_blocking=cuda) for t in b)
                yield b
        finally:                                  # abandoned iterator (zip() of unequal sets, next(iter(..))): release the worker
            stop.set()

    def unbatch(self):
        for f in self.files:
            yield self.make_example(f)


@contextlib.contextmanager
def uncounted_passes(*sets):
    """Passes over `sets` inside the block do not count.  A shuffled Batches / DeviceBatches counts its passes to draw the order of
    the next one; a measurement that walks a set once more (CycleGAN.evaluate between two epochs) must not move the orders of the
    later epochs.  Inside, successive passes still draw successive orders, starting from the one that is due; on the way out the
    counters are back.  Anything else among `sets` (a list of batches, a generator, None) has no order to keep and is left alone."""
    counted = [d for d in sets if isinstance(d, (Batches, DeviceBatches))]
    epochs = [d.epoch for d in counted]
    try:
        yield
    finally:
        for d, epoch in zip(counted, epochs):
            d.epoch = epoch


def chunked(items, n):
    """Consecutive lists of n items (the last one shorter if the items run out)."""
    chunk = []
    for it in items:
        chunk.append(it)
        if len(chunk) == n:
            yield chunk
            chunk = []
    if chunk:
        yield chunk


# ---- device-resident dataset ---------------------------------------------------------------------------
def normalize_table() -> np.ndarray:
    """`normalize` of every byte value: the device path looks the float32 result up instead of recomputing it."""
    return normalize(np.arange(256, dtype=np.float32))


class DeviceDataset:
    """Every file of `files` decoded ONCE to uint8 (the same PIL convert as `load`) and kept in one device buffer, with the index
    tables that restate the host chain for gan_augment_u8 (include/gan_amd.h):
      kind 'pair'   (Pix2Pix): split at w // 2, each half resized by nearest_index(side, L)
      kind 'single' (CycleGAN): resized to size, then to L: the composition nearest_index(side, size)[nearest_index(size, L)]
    with L = size + 30 for the jittered (training) form and L = size for the validation / test form.  One table per distinct
    source side length.  `preprocess_a` / `preprocess_b` (gan_amd/preprocess.py): run once over the resident
    buffer behind the upload, before any batch is built - over the input half (a) and the target half (b) of every pair, or over
    the whole image of kind 'single' (preprocess_a only).  `cap_bytes`: the decoded bytes are added up from the image headers before anything is decoded or
    allocated; more than the cap is an error (no fall-back to the host pipeline)."""

    DECODE_WORKERS = 16

    def __init__(self, files, channels, size, device, kind='pair', jitter=True, orient='left', cap_bytes=64 << 30,
                 preprocess_a=None, preprocess_b=None):
        from PIL import Image
        assert kind in ('pair', 'single') and orient in ('left', 'right') and int(channels) in (1, 3)
        self.files, self.c, self.size, self.device = list(files), int(channels), int(size), device
        self.kind, self.jitter, self.orient = kind, bool(jitter), orient
        self.table_len = self.size + 30 if jitter else self.size
        dims = []
        for f in self.files:
            with Image.open(f) as im:          # header only: nothing is decoded here
                dims.append((im.size[1], im.size[0]))
        align = lambda v: (v + 15) & ~15
        self.offsets, total = [], 0
        for h, w in dims:
            self.offsets.append(total)
            total += align(h * w * self.c)
        self.nbytes = max(total, 16)
        if self.nbytes > cap_bytes:
            raise ValueError(f"--data-cache device: the {len(self.files)} decoded images take {self.nbytes / 2**30:.2f} GiB, more than "
                             f"the cap of {cap_bytes / 2**30:.2f} GiB; raise --data-cache-gb or use --data-cache host")
        # index tables, one per distinct source side length
        tables, ids = [], {}

        def table(n_in):
            if n_in not in ids:
                if kind == 'pair':
                    t = nearest_index(n_in, self.table_len)
                else:
                    t = nearest_index(n_in, self.size)[nearest_index(self.size, self.table_len)]
                ids[n_in] = len(tables)
                tables.append(t.astype(np.int32))
            return ids[n_in]
        self.meta = []          # per file: (byte offset, row pitch, col0 a, col0 b, row table, column table a, column table b)
        for (h, w), off in zip(dims, self.offsets):
            if kind == 'pair':
                half = w // 2
                first, second = (0, half), (half, w - half)            # (first column, width) of the left and the right half
                a, b = (first, second) if orient == 'left' else (second, first)
                self.meta.append((off, w * self.c, a[0], b[0], table(h), table(a[1]), table(b[1])))
            else:
                self.meta.append((off, w * self.c, 0, 0, table(h), table(w), table(w)))
        host = np.zeros(self.nbytes, np.uint8)

        def put(k):
            a = decode(self.files[k], self.c)
            assert a.shape == (dims[k][0], dims[k][1], self.c), (self.files[k], a.shape)
            host[self.offsets[k]:self.offsets[k] + a.size] = a.reshape(-1)
        if self.files:
            from concurrent.futures import ThreadPoolExecutor
            with ThreadPoolExecutor(max_workers=min(self.DECODE_WORKERS, len(self.files))) as pool:
                list(pool.map(put, range(len(self.files))))       # (list: a decode error is raised here)
        import torch
        self.src = torch.from_numpy(host).to(device)                # one upload
        self.tables = torch.from_numpy(np.stack(tables) if tables else np.zeros((1, self.table_len), np.int32)).to(device)
        self.lut = torch.from_numpy(normalize_table()).to(device)
        assert kind == 'pair' or not preprocess_b, "a 'single' dataset has one region per image: preprocess_a"
        # (offset, pitch, first column a, first column b) are the meta's; the sides come from the header sizes
        for pre, col in ((preprocess_a, 2), (preprocess_b, 3)):
            if not pre or (col == 3 and kind != 'pair'):
                continue
            regions = []
            for (h, w), m in zip(dims, self.meta):
                half = w // 2
                width = w if kind == 'single' else (half if m[col] == 0 else w - half)
                regions.append((m[0] + m[col] * self.c, m[1], h, width))
            pre.apply_device(self.src, regions, channels=self.c)      # enqueue-only, chunks of 64 regions inside the call


    def augment(self, idx, draws, out=None):
        """Enqueue the batch of the entries `idx` with the per-example (crop y, crop x, mirror) of `draws` on the current stream:
        one gan_augment_u8 launch per 64 examples.  -> tuple of NHWC float32 tensors (both images of a pair, or the single
        one), freshly allocated unless `out` gives dense 16-byte aligned ones."""
        import torch
        from . import _lib as L
        lib, n, pair = L.load(), len(idx), self.kind == 'pair'
        if out is None:
            out = tuple(torch.empty((n, self.size, self.size, self.c), dtype=torch.float32, device=self.device) for _ in range(2 if pair else 1))
        assert len(out) == (2 if pair else 1) and len(draws) == n
        for t in out:
            assert t.shape == (n, self.size, self.size, self.c) and t.dtype == torch.float32 and t.is_contiguous()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        per = self.size * self.size * self.c * 4
        for lo in range(0, n, L.AUGMENT_MAX_SAMPLES):
            part = idx[lo:lo + L.AUGMENT_MAX_SAMPLES]
            samples = (L.GanAugSample * len(part))()
            for s, k, (y, x, flip) in zip(samples, part, draws[lo:]):
                (s.src_offset, s.src_pitch, s.col0, s.col0_b, s.row_table, s.col_table, s.col_table_b) = self.meta[k]
                s.crop_y, s.crop_x, s.flip = y, x, int(flip)
            d = L.GanAugmentDesc(len(part), self.size, self.c, self.src.data_ptr(), self.nbytes, self.tables.data_ptr(),
                                 self.tables.shape[0], self.table_len, self.lut.data_ptr(), out[0].data_ptr() + lo * per,
                                 out[1].data_ptr() + lo * per if pair else None, ctypes.addressof(samples))
            L.check(lib.gan_augment_u8(ctypes.byref(d), stream), "augment_u8")
        return out


class DeviceBatches:
    """The iteration surface of `Batches` over a DeviceDataset: same file order, same per-epoch reshuffle, last partial batch kept,
    tuples of freshly allocated NHWC float32 device tensors - built by one gan_augment_u8 launch per (at most 64) examples on the
    current stream instead of decode + numpy + upload.  `draw() -> (y, x, flip)` is called once per example in file order, in the
    consuming thread (D.draw_jitter on the model's generator); None = no crop, no mirror.  `make_example` serves unbatch() on the
    host path."""

    def __init__(self, dataset, batch_size, draw=None, shuffle_seed=None, make_example=None):
        assert (draw is not None) == dataset.jitter, "a jittered dataset needs the draws, a plain one takes none"
        self.ds, self.bs, self.draw, self.shuffle_seed, self.make_example = dataset, batch_size, draw, shuffle_seed, make_example
        self.files, self.device, self.epoch = dataset.files, dataset.device, 0
        self.host_seconds = {'draws': 0.0, 'launch': 0.0}       # tools/bench_epoch.py: where the host time of a batch goes

    def __len__(self):
        return (len(self.files) + self.bs - 1) // self.bs

    def _build(self, idx):
        """One batch from the dataset entries `idx`: the draws in file order, then the launches."""
        import time
        t0 = time.perf_counter()
        draws = [self.draw() for _ in idx] if self.draw is not None else [(0, 0, False)] * len(idx)
        t1 = time.perf_counter()
        out = self.ds.augment(idx, draws)
        self.host_seconds['draws'] += t1 - t0
        self.host_seconds['launch'] += time.perf_counter() - t1
        return out

    def __iter__(self):
        order = list(range(len(self.files)))
        if self.shuffle_seed is not None:        # random.sample picks positions: the same permutation as Batches makes of the files
            order = random.Random(self.shuffle_seed + self.epoch).sample(order, len(order))
        self.epoch += 1
        for i in range(0, len(order), self.bs):
            yield self._build(order[i:i + self.bs])

    def unbatch(self):
        for f in self.files:
            yield self.make_example(f)
