#!/usr/bin/env python3
"""Epoch throughput of Pix2Pix training as the CLI feeds it: the host input pipeline against the
device-resident one, beside the bare replay rate of the same captured step on resident inputs.

Writes N synthetic pair PNGs (seeded noise, 256x512 grey by default) to a temporary directory and measures in ONE process:
  (a) one epoch with the host pipeline (gan_amd.data.Batches: decode + numpy + upload per epoch),
  (b) the device pipeline (DeviceDataset + DeviceBatches): build (decode once + upload), first epoch, and the later epochs,
  (c) the captured step replayed on resident inputs (bench.py's quantity) and train_step() on resident inputs,
  (d) the host time of one device-pipeline step split into draws / augment launch / train_step,
  and the augment launch against gan_pack_multi on the same number of output bytes (HIP events).
Prints one JSON line; --out also saves it.  Every timed point runs at least a second after a warm-up and ends in a device sync."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_pairs(d, n, size, channels, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    files = []
    for k in range(n):
        a = rng.integers(0, 256, (size, 2 * size) if channels == 1 else (size, 2 * size, 3), dtype=np.uint8)
        files.append(os.path.join(d, f"{k:05d}.png"))
        Image.fromarray(a).save(files[-1])
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=2048)
    ap.add_argument('--img-size', type=int, default=256)
    ap.add_argument('--channels', type=int, default=1, choices=[1, 3])
    ap.add_argument('--batch-size', type=int, default=16)
    ap.add_argument('--dtype', default='bf16')
    ap.add_argument('--later-epochs', type=int, default=4, help='device-pipeline epochs timed together after the first')
    ap.add_argument('--replay-steps', type=int, default=400)
    ap.add_argument('--seed', type=int, default=123)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    from gan_amd import _lib as L
    from gan_amd import data as D
    from gan_amd import pix2pix
    assert torch.cuda.is_available(), "bench_epoch.py needs an MI355X"
    sync = torch.cuda.synchronize
    res = {'tool': 'bench_epoch', 'model': 'pix2pix', 'n_images': a.n, 'img_size': a.img_size, 'channels': a.channels,
           'batch_size': a.batch_size, 'dtype': a.dtype}
    with tempfile.TemporaryDirectory() as tmp:
        files = write_pairs(tmp, a.n, a.img_size, a.channels, a.seed)
        opt = pix2pix.parse_opt(['--data', tmp, '--output', tmp, '--train', '--epochs', '1', '--batch-size', str(a.batch_size),
                                 '--img-size', str(a.img_size), '--channels', str(a.channels), '--dtype', a.dtype, '--seed', str(a.seed)])
        m = pix2pix.Pix2Pix(vars(opt))
        dev, bs = m.ctx.device, a.batch_size

        def epoch(ds):
            n, acc = 0, None
            for x, y in ds:
                losses = torch.stack(m.train_step(x, y))
                acc = losses if acc is None else acc + losses
                n += x.shape[0]
            acc.cpu()                                   # the drain run_epochs makes per pass
            return n

        # resident inputs; warm-up (captures the steps of the full and of the last partial batch)
        x = torch.rand(bs, a.img_size, a.img_size, a.channels, device=dev) * 2 - 1
        y = torch.rand_like(x) * 2 - 1
        for n in {bs, a.n % bs} - {0}:
            for _ in range(10):
                m.train_step(x[:n], y[:n])
        sync()

        # (c) bare replay and train_step on resident inputs
        _, replay = m._step_for(bs, True)
        for name, fn in (('replay', lambda: replay(x, y)), ('train_step_resident', lambda: m.train_step(x, y))):
            for _ in range(20):
                fn()
            sync()
            t0 = time.perf_counter()
            for _ in range(a.replay_steps):
                fn()
            sync()
            dt = time.perf_counter() - t0
            res[name] = {'steps': a.replay_steps, 'seconds': dt, 'img_per_s': a.replay_steps * bs / dt}

        # (a) host pipeline, one epoch
        host = D.Batches(files, m.process_images_train, bs, dev)
        sync()
        t0 = time.perf_counter()
        n = epoch(host)
        sync()
        dt = time.perf_counter() - t0
        res['host_cache'] = {'epochs': 1, 'seconds': dt, 'img_per_s': n / dt}

        # (b) device pipeline: build, first epoch, later epochs
        t0 = time.perf_counter()
        ds = D.DeviceDataset(files, a.channels, a.img_size, dev, 'pair', True, opt.input_img_orient)
        sync()
        t_build = time.perf_counter() - t0
        devb = D.DeviceBatches(ds, bs, lambda: D.draw_jitter(m._rng), make_example=m.process_images_train)
        t0 = time.perf_counter()
        n = epoch(devb)
        sync()
        t_first = time.perf_counter() - t0
        t0 = time.perf_counter()
        n = sum(epoch(devb) for _ in range(a.later_epochs))
        sync()
        dt = time.perf_counter() - t0
        res['device_cache'] = {'cached_bytes': ds.nbytes, 'build_seconds': t_build, 'first_epoch_seconds_with_build': t_build + t_first,
                               'first_epoch_img_per_s_with_build': a.n / (t_build + t_first), 'later_epochs': a.later_epochs,
                               'later_seconds': dt, 'later_img_per_s': n / dt}

        # (d) host time per step of the device pipeline (no sync inside: what the Python thread spends enqueueing)
        devb.host_seconds = {'draws': 0.0, 'launch': 0.0}
        t_step, steps = 0.0, 0
        sync()
        t0 = time.perf_counter()
        for xb, yb in devb:
            t1 = time.perf_counter()
            torch.stack(m.train_step(xb, yb))
            t_step += time.perf_counter() - t1
            steps += 1
        t_host = time.perf_counter() - t0
        sync()
        t_wall = time.perf_counter() - t0
        us = lambda s: 1e6 * s / steps
        res['device_cache_host_us_per_step'] = {'draws': us(devb.host_seconds['draws']), 'augment_launch': us(devb.host_seconds['launch']),
                                                'train_step': us(t_step), 'python_total': us(t_host), 'wall': us(t_wall)}

        # the augment launch against gan_pack_multi on the same number of output bytes (HIP events, 200 launches each)
        lib = L.load()
        idx, draws = list(range(bs)), [D.draw_jitter(m._rng) for _ in range(bs)]
        out = ds.augment(idx, draws)
        srcs = (C.c_void_p * 2)(out[0].data_ptr(), out[1].data_ptr())
        packed = [torch.empty_like(t) for t in out]
        dsts = (L.GanTensor * 2)(*[L.GanTensor(t.data_ptr(), bs, a.img_size, a.img_size, a.channels, a.channels) for t in packed])
        stream = torch.cuda.current_stream(dev).cuda_stream
        samples = (L.GanAugSample * bs)()
        for sm, k, (cy, cx, flip) in zip(samples, idx, draws):
            (sm.src_offset, sm.src_pitch, sm.col0, sm.col0_b, sm.row_table, sm.col_table, sm.col_table_b) = ds.meta[k]
            sm.crop_y, sm.crop_x, sm.flip = cy, cx, int(flip)
        desc = L.GanAugmentDesc(bs, ds.size, ds.c, ds.src.data_ptr(), ds.nbytes, ds.tables.data_ptr(), ds.tables.shape[0], ds.table_len,
                                ds.lut.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), C.addressof(samples))
        launches = {'gan_augment_u8': lambda: L.check(lib.gan_augment_u8(C.byref(desc), stream), 'augment_u8'),
                    'gan_pack_multi': lambda: L.check(lib.gan_pack_multi(L.F32, 2, srcs, dsts, stream), 'pack_multi')}
        res['launch_us'] = {'output_bytes': 2 * out[0].numel() * 4}
        for name, fn in launches.items():
            for _ in range(20):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            e0.record()
            for _ in range(200):
                fn()
            e1.record()
            sync()
            res['launch_us'][name] = 1e3 * e0.elapsed_time(e1) / 200
        assert torch.equal(out[0], packed[0]) and torch.equal(out[1], packed[1])
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
