#!/usr/bin/env python3
"""Image preprocessing at read-in: what --preprocess-input / --preprocess-target cost at cache build.

    python tools/bench_preprocess.py [--pairs 2048] [--reps 5] [--host-images 4] [--out FILE]

Synthetic grey 512 x 1280 pairs (32 distinct thermal-like images, copied to --pairs files) in a temporary directory.
cache_build  wall seconds of DeviceDataset(...) + synchronize, without preprocessing and with the full chain on both halves
             (decode, upload and, with the chain, the launches over all 2 * pairs regions).
stages       each stage alone and the chain, over all regions of the resident buffer: HIP events around --reps back-to-back
             gan_preprocess_u8 calls with one prepared descriptor and workspace; reported as seconds per call and as region bytes
             per second (every region byte is read and written at least once; the figure counts it once), beside a plain device copy
             of the same number of bytes (counted once as well) measured the same way in the same process.
host         Preprocess.apply_host seconds per pair on one CPU core, full chain on both halves, for scale.
Prints one JSON object; --out also saves it (profiles/bench_preprocess.json).  Reported, not gated."""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def synthetic(k, h=512, w=1280):
    import numpy as np
    rng = np.random.default_rng(k)
    y, x = np.mgrid[0:h, 0:w]
    v = np.full((h, w), 35.0)
    for _ in range(6):
        cy, cx, s, a = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(20, 200), rng.uniform(30, 160)
        v += a * np.exp(-((y - cy) ** 2 + (x - cx) ** 2) / (2 * s * s))
    return np.clip(v + rng.normal(0, 2, (h, w)), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-images', type=int, default=4)
    ap.add_argument('--out', type=str, default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from gan_amd import _lib as L
    from gan_amd import data as D
    from gan_amd.preprocess import Preprocess
    lib, dev = L.load(), 'cuda:0'
    full = Preprocess('clahe,blur,sharpen', 1.0, 15, 0.5)
    tmp = tempfile.mkdtemp(prefix='bench_preprocess_')
    try:
        distinct = min(32, a.pairs)
        for k in range(distinct):
            Image.fromarray(synthetic(k)).save(os.path.join(tmp, f'{k:05d}.png'))
        for k in range(distinct, a.pairs):
            shutil.copy(os.path.join(tmp, f'{k % distinct:05d}.png'), os.path.join(tmp, f'{k:05d}.png'))
        files = [os.path.join(tmp, f) for f in D.list_images(tmp)]
        torch.zeros(1, device=dev)
        torch.cuda.synchronize()
        build = {}
        for name, kw in (('warm_up', {}), ('plain', {}), ('full_chain_both_halves', dict(preprocess_a=full, preprocess_b=full))):
            t0 = time.perf_counter()
            built = D.DeviceDataset(files, 1, 256, dev, 'pair', True, 'left', **kw)
            torch.cuda.synchronize()
            build[name] = time.perf_counter() - t0
            if name == 'plain':
                ds = built              # the buffer the stage timings below run over
            del built
        del build['warm_up']
        regions = []
        for off in ds.offsets:
            regions += [(off, 1280, 512, 640), (off + 640, 1280, 512, 640)]
        nbytes = len(regions) * 512 * 640
        stream = torch.cuda.current_stream().cuda_stream
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            start.record()
            for _ in range(a.reps):
                fn()
            end.record()
            torch.cuda.synchronize()
            return start.elapsed_time(end) * 1e-3 / a.reps

        stages = {}
        for chain in ('clahe', 'blur', 'sharpen', 'clahe,blur,sharpen'):
            pre = Preprocess(chain, 1.0, 15, 0.5)
            d, keep = pre.descriptor(1, regions, ds.src.data_ptr(), ds.src.numel())
            need = lib.gan_preprocess_workspace_bytes(C.byref(d))
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
            d.workspace, d.workspace_bytes = ws.data_ptr(), need
            sec = timed(lambda: L.check(lib.gan_preprocess_u8(C.byref(d), stream), "preprocess_u8"))
            stages[chain] = {'seconds_per_call': sec, 'region_bytes_per_second': nbytes / sec, 'workspace_bytes': need}
        src, dst = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
        sec = timed(lambda: dst.copy_(src))
        copy = {'seconds_per_call': sec, 'bytes_per_second': nbytes / sec}
        imgs = [D.decode(f, 1) for f in files[:a.host_images]]
        t0 = time.perf_counter()
        for img in imgs:
            full.apply_host(img, [(0, 0, 512, 640), (0, 640, 512, 640)])
        host = (time.perf_counter() - t0) / max(len(imgs), 1)
        out = {'pairs': a.pairs, 'pair_shape': [512, 1280], 'regions': len(regions), 'region_bytes': nbytes, 'reps': a.reps,
               'device': torch.cuda.get_device_name(0), 'cache_build_seconds': build, 'stages': stages, 'device_copy': copy,
               'apply_host_seconds_per_pair': host}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(json.dumps(out, indent=1))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(out, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
