#!/usr/bin/env python3
"""Cost of the generator weight average at Pix2Pix 256^2, bf16, batch 16, captured step.

    python tools/bench_ema.py [--min-seconds 1.0] [--pairs 4] [--batch 16] [--out profiles/bench_ema.json]

(a) step: ms per replayed training step with the average detached (st.ema = ()) and attached, the SAME captured step object,
    in alternating windows (--pairs of them, each >= --min-seconds after warm-up, HIP events around the window).
(b) kernel: gan_ema_update over the generator's arena alone, back to back, HIP events; bytes = 12 per element (shadow read and
    written, weights read).
(c) copy: in the same process, a device-to-device copy of an fp32 buffer of the arena's size; bytes = 8 per element.
(b) and (c) alternate as well.  The acceptance criterion compares bytes/s: kernel >= 0.8 x copy.  Prints one JSON object; --out
also saves it.  The step cost is reported, not gated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

from bench_infer import timed  # noqa: E402
from gan_amd.base_gan import GeneratorModel  # noqa: E402
from gan_amd.ema import WeightAverage  # noqa: E402
from gan_amd.nets import Ctx, workspace_mb_for  # noqa: E402
from gan_amd.steps import Pix2PixStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--pairs', type=int, default=4)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--decay', type=float, default=0.999)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ema.py needs an MI355X"
    B = a.batch
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=workspace_mb_for(B, 256, 1))
    st = Pix2PixStep(ctx, B, 256, 1, lam=100.0, seed=123)
    replay = st.capture(training=True)
    ema = WeightAverage(GeneratorModel(st.G), a.decay, True)
    x, y = (torch.rand(B, 256, 256, 1, device=ctx.device) * 2 - 1 for _ in range(2))
    n = st.G.params.total
    res = {'tool': 'bench_ema', 'min_seconds': a.min_seconds, 'pairs': a.pairs, 'device': torch.cuda.get_device_name(0),
           'size': 256, 'batch': B, 'dtype': 'bf16', 'decay': a.decay, 'warmup': True, 'arena_elements': n,
           'step': {'off_ms': [], 'on_ms': []}, 'kernel_us': [], 'copy_us': []}
    for _ in range(a.pairs):
        for key, attached in (('off_ms', ()), ('on_ms', (ema,))):
            st.ema = attached
            ms, _ = timed(lambda: replay(x, y), a.min_seconds)
            res['step'][key].append(ms)
    st.ema = ()
    src, dst = torch.empty(n, device=ctx.device).normal_(), torch.empty(n, device=ctx.device)
    for _ in range(a.pairs):
        ms, _ = timed(ema.update, a.min_seconds / 2)
        res['kernel_us'].append(1e3 * ms)
        ms, _ = timed(lambda: dst.copy_(src), a.min_seconds / 2)
        res['copy_us'].append(1e3 * ms)
    off, on = statistics.median(res['step']['off_ms']), statistics.median(res['step']['on_ms'])
    k_us, c_us = statistics.median(res['kernel_us']), statistics.median(res['copy_us'])
    res['step'].update(off_ms_median=off, on_ms_median=on, cost_ms=on - off, cost_percent=100.0 * (on - off) / off,
                       off_img_s=B * 1e3 / off, on_img_s=B * 1e3 / on)
    res['kernel_bytes'], res['copy_bytes'] = 12 * n, 8 * n
    res['kernel_bytes_per_s'] = 12 * n / (k_us * 1e-6)
    res['copy_bytes_per_s'] = 8 * n / (c_us * 1e-6)
    res['kernel_over_copy'] = res['kernel_bytes_per_s'] / res['copy_bytes_per_s']
    res['criterion'] = 'kernel_over_copy >= 0.8'
    res['criterion_met'] = bool(res['kernel_over_copy'] >= 0.8)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
