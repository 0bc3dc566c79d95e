"""Image preprocessing on the GPU: gan_preprocess_u8 against Preprocess.apply_host, DeviceDataset with
preprocess_a / preprocess_b against the host chain, and the command line with either --data-cache.  Every comparison is exact
(torch.equal / ==): both sides are integer work plus one fp32 blend that rounds every operation on its own."""
import ctypes as C
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gan_amd import data as D
from gan_amd.preprocess import Preprocess

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = 'cuda:0'
CHAINS = ('clahe', 'blur', 'sharpen', 'clahe,blur,sharpen')
# the staging budget of the CLAHE apply kernel (gan_amd/csrc/preprocess.hip: PRE_LUT_LDS): two table rows of every channel,
# 2 * c * grid * 256 bytes, are kept in LDS up to this size and read from the workspace beyond it
PRE_LUT_LDS = 32768


def _image(kind, h, w, c, seed):
    rng = np.random.default_rng(seed)
    if kind == 'random':
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == 'constant':
        return np.full((h, w, c), 93, np.uint8)
    if kind == 'two':
        return np.where(rng.random((h, w, c)) < 0.3, 200, 17).astype(np.uint8)
    if kind == 'ramp':
        return np.broadcast_to(((np.arange(w)[None, :] * 3 + np.arange(h)[:, None]) % 256).astype(np.uint8)[..., None], (h, w, c)).copy()
    if kind == 'smooth':             # thermal-like: a few blobs on a flat background
        y, x = np.mgrid[0:h, 0:w]
        v = 40 + sum(a * np.exp(-((y - cy * h) ** 2 + (x - cx * w) ** 2) / (2 * (s * w) ** 2))
                     for a, cy, cx, s in ((150, .3, .3, .1), (90, .7, .6, .2), (60, .5, .9, .05)))
        return np.broadcast_to(np.clip(v, 0, 255).astype(np.uint8)[..., None], (h, w, c)).copy()
    raise KeyError(kind)


def _pack(images, extra_pitch, seed=1):
    """The images in one byte buffer the way a caller may hold them: a row pitch of width * c + extra_pitch bytes, odd gaps before,
    between and behind them, everything that is not a pixel filled with random bytes.  -> (buffer, [(offset, pitch)])"""
    rng = np.random.default_rng(seed)
    where, total = [], 37
    for img in images:
        h, w, c = img.shape
        pitch = w * c + extra_pitch
        where.append((total, pitch))
        total += h * pitch + 29
    buf = rng.integers(0, 256, total + 16, dtype=np.uint8)
    for img, (off, pitch) in zip(images, where):
        h, w, c = img.shape
        rows = buf[off:off + h * pitch].reshape(h, pitch)
        rows[:, :w * c] = img.reshape(h, w * c)
    return buf, where


def _expect(pre, buf, images, where, regions):
    """The buffer with the regions (image number, y0, x0, h, w) replaced by apply_host's bytes; everything else as it was."""
    want = buf.copy()
    for k, (img, (off, pitch)) in enumerate(zip(images, where)):
        h, w, c = img.shape
        rows = want[off:off + h * pitch].reshape(h, pitch)
        done = pre.apply_host(rows[:, :w * c].reshape(h, w, c), [r[1:] for r in regions if r[0] == k])
        rows[:, :w * c] = done.reshape(h, w * c)
    return want


def _device_regions(images, where, regions):
    return [(where[k][0] + y0 * where[k][1] + x0 * images[k].shape[2], where[k][1], h, w) for k, y0, x0, h, w in regions]


def _check(pre, images, regions, extra_pitch=0):
    buf, where = _pack(images, extra_pitch)
    want = _expect(pre, buf, images, where, regions)
    dev = torch.from_numpy(buf.copy()).to(DEV)
    pre.apply_device(dev, _device_regions(images, where, regions), channels=images[0].shape[2])
    got = dev.cpu()
    if not torch.equal(got, torch.from_numpy(want)):
        bad = np.flatnonzero(got.numpy() != want)
        raise AssertionError(f"{pre}: {bad.size} bytes differ, first at {bad[:5]}: got {got.numpy()[bad[:5]]}, want {want[bad[:5]]}")


# (id, image kind, H, W, c, regions (y0, x0, h, w), clip, grid, sigma, extra pitch)
SMALL = [
    ('37x53-offset-pitch', 'random', 41, 64, 1, [(2, 7, 37, 53)], 1.0, 15, 0.5, 5),
    ('16x16-grid4-clip40', 'random', 16, 16, 1, [(0, 0, 16, 16)], 40.0, 4, 0.5, 0),
    ('16x16-grid-is-width', 'two', 16, 16, 1, [(0, 0, 16, 16)], 1.0, 16, 1.0, 3),
    ('15x31-grid15-noclip', 'ramp', 15, 31, 1, [(0, 0, 15, 31)], 0.0, 15, 0.5, 1),
    ('15x31-tiny-tiles', 'random', 15, 31, 3, [(0, 0, 15, 31)], 1.0, 15, 1.5, 0),      # area 3: int(clip * area / 256) == 0
    ('37x53-grid1-rgb', 'random', 37, 53, 3, [(0, 0, 37, 53)], 1.0, 1, 1.0, 2),
    ('constant-64x80', 'constant', 64, 80, 1, [(0, 0, 64, 80)], 1.0, 4, 0.5, 0),         # every lane on one histogram bin
    ('pair-257x511', 'random', 257, 511, 1, [(0, 0, 257, 255), (0, 255, 257, 256)], 1.0, 15, 0.5, 0),
    ('pair-257x511-rgb', 'smooth', 257, 511, 3, [(0, 0, 257, 255), (0, 255, 257, 256)], 2.0, 8, 1.0, 0),
    ('grid32-rgb-over-budget', 'random', 45, 70, 3, [(0, 0, 45, 70)], 3.0, 32, 0.5, 0),
    ('frame-512x640', 'smooth', 512, 640, 1, [(0, 0, 512, 640)], 1.0, 15, 0.5, 0),
]


@pytest.mark.parametrize('chain', CHAINS)
@pytest.mark.parametrize('case', SMALL, ids=[s[0] for s in SMALL])
def test_kernels_match_apply_host_byte_for_byte(case, chain):
    """Each stage alone and the chain of all three, over the whole buffer: the regions equal apply_host, and the gaps, the row
    remainders and whatever lies outside the regions keep their bytes."""
    _, kind, H, W, c, regions, clip, grid, sigma, extra = case
    img = _image(kind, H, W, c, seed=H * 31 + W)
    _check(Preprocess(chain, clip, grid, sigma), [img], [(0,) + r for r in regions], extra)


def test_the_cases_sit_on_the_seams_they_are_meant_for():
    rgb = next(s for s in SMALL if s[0] == 'grid32-rgb-over-budget')
    assert 2 * rgb[4] * rgb[7] * 256 > PRE_LUT_LDS >= 2 * 3 * 15 * 256        # grid 32 x 3 channels: 48 KiB, not staged
    frame = next(s for s in SMALL if s[0] == 'frame-512x640')
    tw, th = -(-640 // 15), -(-512 // 15)
    assert (tw, th, tw * 15, th * 15) == (43, 35, 645, 525) and max(int(1.0 * tw * th / 256), 1) == 5
    assert frame[6:8] == (1.0, 15)
    assert max(int(1.0 * 3 * 1 / 256), 1) == 1 and int(1.0 * 3 / 256) == 0          # 15x31 at grid 15: tiles of 3 x 1


def test_one_half_of_a_pair_leaves_the_other_alone():
    """Only half A is a region: half B, the gaps and the row remainder keep their bytes (the whole-buffer comparison of _check)."""
    img = _image('random', 64, 130, 1, seed=4)
    for chain in CHAINS:
        _check(Preprocess(chain, 1.0, 8, 0.5), [img], [(0, 0, 0, 64, 65)], 6)
        _check(Preprocess(chain, 1.0, 8, 0.5), [img], [(0, 0, 65, 64, 65)], 6)


def test_65_regions_in_one_call_are_two_launches_and_complete():
    images = [_image('random' if k % 3 else 'two', 20 + k % 7, 24 + k % 5, 1, seed=k) for k in range(65)]
    regions = [(k, 0, 0) + images[k].shape[:2] for k in range(65)]
    assert len(regions) > 64              # GAN_PREPROCESS_MAX_REGIONS per launch
    _check(Preprocess('clahe,blur,sharpen', 1.0, 4, 0.5), images, regions, 0)


def test_bad_descriptors_are_refused_and_nothing_is_written():
    from gan_amd import _lib as L
    lib = L.load()
    img = _image('random', 40, 48, 1, seed=2)
    buf, where = _pack([img], 0)
    dev = torch.from_numpy(buf.copy()).to(DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(pre=None, regions=None, c=1, null_regions=False, **fields):
        pre = pre or Preprocess('clahe,blur,sharpen', 1.0, 8, 0.5)
        regions = regions or [(where[0][0], where[0][1], 40, 48)]
        d, keep = pre.descriptor(c, regions, dev.data_ptr(), dev.numel())
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
        for k, v in fields.items():
            setattr(d, k, v)
        if null_regions:
            d.regions = None
        return lib.gan_preprocess_u8(C.byref(d), stream)

    off, pitch = where[0]
    assert lib.gan_preprocess_u8(None, stream) == L.E_ARG
    assert call(struct_size=C.sizeof(L.GanPreprocessDesc) - 8) == L.E_ARG
    for ptr in ('src', 'workspace'):
        assert call(**{ptr: None}) == L.E_ARG, ptr
    assert call(null_regions=True) == L.E_ARG
    assert call(workspace=ws.data_ptr() + 4) == L.E_ARG                      # not 16-byte aligned
    assert call(n=0) == L.E_ARG and call(stages=0) == L.E_ARG and call(stages=8) == L.E_ARG
    for c in (0, 2, 4):
        assert call(c=c) == L.E_ARG
    assert call(regions=[(dev.numel() - 100, pitch, 40, 48)]) == L.E_ARG     # runs past the end of src
    assert call(regions=[(-1, pitch, 40, 48)]) == L.E_ARG
    assert call(regions=[(off, 47, 40, 48)]) == L.E_ARG                      # pitch < width * c
    assert call(src_bytes=off + 39 * pitch + 47) == L.E_ARG                  # one byte short of the last row
    for grid in (0, 33, -1):
        assert call(grid=grid) == L.E_ARG
    for sigma in (0.0, -1.0, 1.6, float('nan')):
        assert call(sigma=sigma) == L.E_ARG
    for clip in (-0.5, float('inf'), float('nan')):
        assert call(clip=clip) == L.E_ARG
    assert call(regions=[(off, pitch, 7, 48)]) == L.E_SHAPE                  # a side shorter than grid 8
    assert call(regions=[(off, pitch, 40, 7)]) == L.E_SHAPE
    assert call(Preprocess('blur', sigma=1.5), regions=[(off, pitch, 5, 48)]) == L.E_SHAPE        # r = 5: sides >= 6
    assert call(Preprocess('sharpen'), regions=[(off, pitch, 1, 48)]) == L.E_SHAPE
    d, keep = Preprocess('clahe,blur,sharpen', 1.0, 8, 0.5).descriptor(1, [(off, pitch, 40, 48)])
    need = lib.gan_preprocess_workspace_bytes(C.byref(d))
    assert need == 8 * 8 * 256 + 40 * 48                                     # the tile tables and one dense copy
    assert call(workspace_bytes=need - 1) == L.E_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(dev.cpu(), torch.from_numpy(buf)) and not bool(ws.any())
    assert call(workspace_bytes=need) == 0                                   # ... and the good descriptor runs
    torch.cuda.synchronize()
    assert not torch.equal(dev.cpu(), torch.from_numpy(buf))


# ---- DeviceDataset --------------------------------------------------------------------------------------------------------------
def _png(path, a):
    from PIL import Image
    Image.fromarray(a[..., 0] if a.shape[2] == 1 else a).save(path)
    return path


def _host_example(f, c, size, kind, orient, draw, pa, pb):
    """The host chain with the preprocessing in front of the cast: decode -> apply_host per region -> split | resize -> ..."""
    img = D.decode(f, c)
    H, W = img.shape[:2]
    if kind == 'pair':
        first, second = (0, 0, H, W // 2), (0, W // 2, H, W - W // 2)
        ra, rb = (first, second) if orient == 'left' else (second, first)
        img = pb.apply_host(pa.apply_host(img, [ra]), [rb])
        parts = D.split_img(img.astype(np.float32), orient)
    else:
        parts = (D.resize_nearest(pa.apply_host(img).astype(np.float32), size, size),)
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


@pytest.mark.parametrize('c', [1, 3])
def test_device_dataset_batches_equal_the_host_chain(tmp_path, c):
    sizes = [(40, 100), (257, 511), (300, 600), (64, 3000)]              # odd sizes of tests/test_gpu_device_data.py
    files = [_png(str(tmp_path / f'{k}.png'), _image('random' if k % 2 else 'smooth', h, w, c, seed=k)) for k, (h, w) in enumerate(sizes)]
    pa, pb = Preprocess('clahe,blur,sharpen', 1.0, 15, 0.5), Preprocess('clahe', 2.0, 15, 0.5)
    draws = [(0, 0, False), (30, 30, True), (17, 5, False), (3, 29, True)]
    size = 256
    for kind, orients in (('pair', ('left', 'right')), ('single', ('left',))):
        for orient in orients:
            kw = dict(preprocess_a=pa, preprocess_b=pb) if kind == 'pair' else dict(preprocess_a=pa)
            ds = D.DeviceDataset(files, c, size, DEV, kind, True, orient, **kw)
            it = iter(draws)
            (got,) = list(D.DeviceBatches(ds, len(files), lambda: next(it)))
            plain = D.DeviceDataset(files, c, size, DEV, kind, False, orient, **kw)
            (got_plain,) = list(D.DeviceBatches(plain, len(files)))
            for k, f in enumerate(files):
                for g, w in zip(got, _host_example(f, c, size, kind, orient, draws[k], pa, pb)):
                    assert torch.equal(g[k].cpu(), torch.from_numpy(np.ascontiguousarray(w))), (kind, orient, k)
                for g, w in zip(got_plain, _host_example(f, c, size, kind, orient, None, pa, pb)):
                    assert torch.equal(g[k].cpu(), torch.from_numpy(np.ascontiguousarray(w))), (kind, orient, k, 'plain')
    # without the arguments the buffer holds the decoded bytes, as before
    ds = D.DeviceDataset(files[:1], c, size, DEV, 'pair', False, 'left')
    assert torch.equal(ds.src[:40 * 100 * c].cpu(), torch.from_numpy(D.decode(files[0], c).reshape(-1).copy()))


# ---- command line ---------------------------------------------------------------------------------------------------------------
FLAGS = ['--preprocess-input', 'clahe,blur,sharpen', '--preprocess-target', 'clahe']


def _find(out, name):
    (path,) = glob.glob(os.path.join(out, '**', name), recursive=True)
    return path


def test_cli_trains_alike_with_either_cache_and_prediction_sees_the_flags(tmp_path):
    from gan_amd import pix2pix
    data = str(tmp_path / 'data')
    os.makedirs(data)
    for k in range(8):
        _png(os.path.join(data, f'{k}.png'), _image('smooth' if k % 2 else 'random', 256, 512, 1, seed=700 + k))
    metrics = {}
    for cache in ('host', 'device'):                      # two child processes, one after the other
        out = str(tmp_path / f'out_{cache}')
        cmd = [sys.executable, os.path.join(ROOT, 'pix2pix.py'), '--data', data, '--output', out, '--train', '--epochs', '1', '--batch-size', '1',
               '--test-img', '2', '--dtype', 'bf16', '--data-cache', cache, '--logging', 'false',
               '--save-weights', 'true' if cache == 'device' else 'false'] + FLAGS
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, (cache, r.stdout[-2000:], r.stderr[-3000:])
        for name in ('train_metrics.json', 'val_metrics.json'):
            metrics[cache, name] = json.load(open(_find(out, name)))
        cfg = json.load(open(_find(out, 'config.json')))
        assert cfg['preprocess_input'] == 'clahe,blur,sharpen' and cfg['preprocess_target'] == 'clahe'
        assert (cfg['clahe_clip'], cfg['clahe_grid'], cfg['blur_sigma']) == (1.0, 15, 0.5)
    for name in ('train_metrics.json', 'val_metrics.json'):
        assert metrics['host', name], name
        assert metrics['host', name] == metrics['device', name], (name, metrics['host', name], metrics['device', name])
    ck = _find(str(tmp_path / 'out_device'), 'training_checkpoints')
    pm = {}
    for tag, flags in (('first', FLAGS), ('second', FLAGS), ('none', [])):
        out = str(tmp_path / f'predict_{tag}')
        pix2pix.main(pix2pix.parse_opt(['--data', data, '--predict', '--weights', ck, '--logging', 'false', '--output', out,
                                        '--predict-resolution', 'resized', '--predict-training', 'false', '--quality-metrics', 'true'] + flags))
        pm[tag] = json.load(open(_find(out, 'prediction_metrics.json')))['per_image']
        cfg = json.load(open(_find(out, 'config.json')))
        assert cfg['preprocess_input'] == (flags[1] if flags else '')
    assert pm['first'] == pm['second']
    assert pm['first'] != pm['none']                       # the flags reach prediction: other inputs, other targets, other metrics
