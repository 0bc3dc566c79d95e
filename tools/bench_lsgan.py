#!/usr/bin/env python3
"""The captured training step with gan_loss 'lsgan' beside 'bce' (DESIGN.md section 16), for information: Pix2Pix bf16 256^2 at
--p2p-batch and CycleGAN bf16 256^2 at --cyc-batch, same seeds and inputs, the adversarial loss alone differs.

    python tools/bench_lsgan.py [--min-seconds 1.0] [--p2p-batch 16] [--cyc-batch 1] [--out FILE]

Every point: warm-up, then HIP events around as many back-to-back replays as fill --min-seconds (tools/bench_infer.py's `timed`),
the two losses interleaved, two windows each.  Prints one JSON object; --out also saves it.  Reported, not gated: whether the default
path costs anything is decided by bench.py on this commit against its parent (profiles/bench_lsgan.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

from bench_infer import timed  # noqa: E402
from gan_amd.nets import Ctx  # noqa: E402
from gan_amd.steps import CycleGANStep, Pix2PixStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--p2p-batch', type=int, default=16)
    ap.add_argument('--cyc-batch', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lsgan.py needs an MI355X"
    res = {'tool': 'bench_lsgan', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'dtype': 'bf16', 'size': 256}
    for model, B in (('pix2pix', a.p2p_batch), ('cyclegan', a.cyc_batch)):
        ctx = Ctx('cuda:0', 'bf16')
        x, y = (torch.rand(B, 256, 256, 1, device=ctx.device) * 2 - 1 for _ in range(2))
        point = res[model] = {'batch': B}
        for kind in ('bce', 'lsgan', 'bce', 'lsgan'):
            if model == 'pix2pix':
                st = Pix2PixStep(ctx, B, 256, 1, lam=100.0, seed=123, gan_loss=kind)
            else:
                st = CycleGANStep(ctx, B, 256, 1, lam=10.0, seed=123, gan_loss=kind)
            replay = st.capture(training=True)
            ms, n = timed(lambda: replay(x, y), a.min_seconds)
            point.setdefault(kind + '_ms', []).append(ms)
            point.setdefault(kind + '_losses', []).append([float(v) for v in st.losses[:4].cpu()])
            del st, replay
            torch.cuda.empty_cache()
        del ctx
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
