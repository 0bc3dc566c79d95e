"""The device-resident input pipeline on the GPU: gan_augment_u8 and DeviceDataset / DeviceBatches against
the host chain of gan_amd/data.py.  Every comparison is torch.equal - both sides are an integer gather and one float32 table
value, so there is no tolerance anywhere in this file."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gan_amd import data as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'

# (height, width) of the PNGs.  248x496 and 312x624 have half-image sides where floor((d + .5) * in / out) in float64 and the integer
# form differ at 286 outputs, 304x608 at 542; 257x511 has halves of different widths; the last two are wider than the kernel's
# LDS staging budget (4,096 bytes of source row) with 3 and with 1 channel: the global-gather form
SIZES = [(40, 100), (256, 512), (300, 600), (257, 511), (600, 1200), (248, 496), (312, 624), (304, 608), (64, 3000), (48, 9000)]
CROPS = [(0, 0), (30, 30), (0, 30), (17, 5)]
DRAWS = [(y, x, flip) for (y, x) in CROPS for flip in (False, True)]


def _png(path, h, w, c, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w) if c == 1 else (h, w, 3), dtype=np.uint8)
    Image.fromarray(a).save(path)
    return path


def _host(f, c, size, kind, orient, draw):
    """The host chain: load -> split | resize to size -> resize to size+30 -> crop -> mirror -> normalize (draw None: the
    validation form, resize to size only)."""
    img = D.load(f, c)
    parts = D.split_img(img, orient) if kind == 'pair' else (D.resize_nearest(img, size, size),)
    out = []
    for p in parts:
        if draw is None:
            p = D.resize_nearest(p, size, size)
        else:
            y, x, flip = draw
            p = D.resize_nearest(p, size + 30, size + 30)[y:y + size, x:x + size]
            p = p[:, ::-1] if flip else p
        out.append(D.normalize(p))
    return out


def _scripted(draws):
    it = iter(draws)
    return lambda: next(it)


@pytest.mark.parametrize('c', [1, 3])
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernel_matches_the_host_chain(tmp_path, hw, c):
    f = _png(str(tmp_path / 'a.png'), hw[0], hw[1], c, seed=hw[0] * 7 + c)
    checked = 0
    for size in (256, 512):
        for kind, orients in (('pair', ('left', 'right')), ('single', ('left',))):
            for orient in orients:
                # jittered form: every crop origin, mirrored and not, in one batch
                ds = D.DeviceDataset([f] * len(DRAWS), c, size, DEV, kind, True, orient)
                (got,) = list(D.DeviceBatches(ds, len(DRAWS), _scripted(DRAWS)))
                assert len(got) == (2 if kind == 'pair' else 1)
                for k, draw in enumerate(DRAWS):
                    want = _host(f, c, size, kind, orient, draw)
                    for g, w in zip(got, want):
                        assert g.dtype == torch.float32 and g.shape == (len(DRAWS), size, size, c)
                        assert torch.equal(g[k].cpu(), torch.from_numpy(np.ascontiguousarray(w))), (hw, c, size, kind, orient, draw)
                        checked += 1
                # validation / test form: resize to size, no crop, no mirror
                ds = D.DeviceDataset([f], c, size, DEV, kind, False, orient)
                (got,) = list(D.DeviceBatches(ds, 4))
                for g, w in zip(got, _host(f, c, size, kind, orient, None)):
                    assert torch.equal(g[0].cpu(), torch.from_numpy(np.ascontiguousarray(w))), (hw, c, size, kind, orient)
                    checked += 1
    assert checked == 2 * 5 * (len(DRAWS) + 1)          # two sizes x (pair left: 2, pair right: 2, single: 1) tensors


def test_sizes_include_indices_where_float64_and_integer_forms_differ():
    """The cases above do cover the sizes the exactness argument is about."""
    for n_in, n_out in ((124, 286), (248, 286), (312, 286), (304, 542)):
        assert not np.array_equal(D.nearest_index(n_in, n_out), ((2 * np.arange(n_out) + 1) * n_in) // (2 * n_out)), (n_in, n_out)
    halves = {w // 2 for _, w in SIZES} | {h for h, _ in SIZES}
    assert {248, 312, 304} <= halves


@pytest.mark.parametrize('c,size', [(1, 256), (3, 256), (1, 512)])
def test_guards_stay_and_70_samples_are_complete(tmp_path, c, size):
    """dst between guard regions of a NaN pattern: nothing outside dst is written; n = 70 (64 + 6: two launches) is complete."""
    n, guard = 70, 1 << 16
    files = [_png(str(tmp_path / f'{k}.png'), 60 + 3 * k, 130 + 2 * k, c, seed=k) for k in range(5)]
    rng = np.random.default_rng(5)
    idx = [int(v) for v in rng.integers(0, len(files), n)]
    draws = [D.draw_jitter(rng) for _ in range(n)]
    ds = D.DeviceDataset(files, c, size, DEV, 'pair', True, 'left')
    per = size * size * c
    pattern = torch.tensor([0x7fc0dead], dtype=torch.int32).view(torch.float32).item()
    buf = torch.full((3 * guard + 2 * n * per,), pattern, dtype=torch.float32, device=DEV)
    bits = buf.view(torch.int32)
    a = buf[guard:guard + n * per].view(n, size, size, c)
    b = buf[2 * guard + n * per:2 * guard + 2 * n * per].view(n, size, size, c)
    ds.augment(idx, draws, out=(a, b))
    torch.cuda.synchronize()
    for lo in (0, guard + n * per, 2 * guard + 2 * n * per):
        assert bool((bits[lo:lo + guard] == 0x7fc0dead).all()), lo
    assert not bool(torch.isnan(a).any()) and not bool(torch.isnan(b).any())
    ah, bh = a.cpu(), b.cpu()
    for k in range(n):
        wa, wb = _host(files[idx[k]], c, size, 'pair', 'left', draws[k])
        assert torch.equal(ah[k], torch.from_numpy(np.ascontiguousarray(wa))) and torch.equal(bh[k], torch.from_numpy(np.ascontiguousarray(wb))), k


class _Model:
    """The part of Pix2Pix / CycleGAN the input pipeline touches: a generator and the host example functions."""

    def __init__(self, seed, c, size):
        self.rng, self.c, self.size = np.random.default_rng(seed), c, size

    def pair_train(self, f):
        a, b = D.random_jitter_pair(*D.split_img(D.load(f, self.c), 'left'), self.size, self.rng)
        return D.normalize(a), D.normalize(b)

    def single_train(self, f):
        return (D.normalize(D.random_jitter_single(D.resize_nearest(D.load(f, self.c), self.size, self.size), self.size, self.rng)),)


@pytest.mark.parametrize('kind', ['pair', 'single'])
@pytest.mark.parametrize('shuffle_seed', [None, 11])
def test_device_batches_equal_batches_over_two_epochs(tmp_path, kind, shuffle_seed):
    c, size, bs = 1, 256, 4
    files = [_png(str(tmp_path / f'{k:02d}.png'), 50 + k, 120 + 2 * k, c, seed=100 + k) for k in range(10)]       # 10 = 4 + 4 + 2
    host_m, dev_m = _Model(9, c, size), _Model(9, c, size)
    host = D.Batches(files, host_m.pair_train if kind == 'pair' else host_m.single_train, bs, DEV, shuffle_seed=shuffle_seed)
    dev = D.DeviceBatches(D.DeviceDataset(files, c, size, DEV, kind, True, 'left'), bs, lambda: D.draw_jitter(dev_m.rng), shuffle_seed)
    assert len(host) == len(dev) == 3
    firsts = []
    for epoch in range(2):
        hb, db = list(host), list(dev)
        assert len(hb) == len(db) == 3 and host.epoch == dev.epoch == epoch + 1
        for h, d in zip(hb, db):
            assert len(h) == len(d) == (2 if kind == 'pair' else 1)
            for th, td in zip(h, d):
                assert td.device == th.device and td.dtype == th.dtype == torch.float32 and td.shape == th.shape
                assert torch.equal(th, td)
        assert db[-1][0].shape[0] == 2
        firsts.append(db[0][0].clone())
    assert not torch.equal(firsts[0], firsts[1])           # new draws (and a new order) in the second epoch


def test_each_file_is_decoded_once_over_three_epochs(tmp_path, monkeypatch):
    files = [_png(str(tmp_path / f'{k}.png'), 64, 128, 3, seed=k) for k in range(6)]
    counts = {}
    real = D.decode

    def counting(f, channels):
        counts[f] = counts.get(f, 0) + 1
        return real(f, channels)
    monkeypatch.setattr(D, 'decode', counting)
    rng = np.random.default_rng(3)
    dev = D.DeviceBatches(D.DeviceDataset(files, 3, 256, DEV, 'pair', True, 'left'), 4, lambda: D.draw_jitter(rng), shuffle_seed=1)
    for _ in range(3):
        assert sum(b[0].shape[0] for b in dev) == len(files)
    assert counts == {f: 1 for f in files}
    # the host pipeline, for contrast, decodes every file in every epoch (through the same function)
    counts.clear()
    host = D.Batches(files, lambda f: (D.load(f, 3),), 4)
    for _ in range(3):
        list(host)
    assert counts == {f: 3 for f in files}


def test_training_is_identical_with_either_cache(tmp_path):
    """pix2pix.py --train twice, once per --data-cache: identical batches into a deterministic captured step give equal metrics."""
    data = str(tmp_path / 'data')
    os.makedirs(data)
    for k in range(24):
        _png(os.path.join(data, f'{k:02d}.png'), 256, 512, 1, seed=500 + k)
    metrics = {}
    for cache in ('host', 'device'):                      # two child processes, one after the other
        out = str(tmp_path / f'out_{cache}')
        cmd = [sys.executable, os.path.join(ROOT, 'pix2pix.py'), '--data', data, '--output', out, '--train', '--epochs', '2', '--batch-size', '4',
               '--dtype', 'bf16', '--data-cache', cache, '--logging', 'false', '--save-weights', 'false']
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (cache, r.stdout[-2000:], r.stderr[-3000:])
        for name in ('train_metrics.json', 'val_metrics.json'):
            (path,) = glob.glob(os.path.join(out, '**', name), recursive=True)
            metrics[cache, name] = json.load(open(path))
    for name in ('train_metrics.json', 'val_metrics.json'):
        assert metrics['host', name], name
        assert metrics['host', name] == metrics['device', name], (name, metrics['host', name], metrics['device', name])
