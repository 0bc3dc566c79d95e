#!/usr/bin/env python3
"""Cost of the dSSIM generator loss: one `gan_dssim` call with its gradient and loss-only, beside one `gan_l1`
call (with its gradient) and one `gan_image_quality` call on the same operands, at the shapes of section 12's table; and the captured
Pix2Pix training step at 256^2 bf16 with generator_loss 'dssim' against 'l1' (for information).

    python tools/bench_dssim.py [--min-seconds 1.0] [--step-batch 16] [--out profiles/bench_dssim.json]

Every point: warm-up, then HIP events around as many back-to-back calls as fill --min-seconds (tools/bench_infer.py's `timed`).
All operands in the step's layout: typed (bf16), 8-channel-padded buffers - gan_l1 takes one dtype, and the step hands gan_dssim
the same two views.  Prints one JSON object; --out also saves it.  Reported, not gated."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

from bench_infer import timed  # noqa: E402
from gan_amd import _lib as L  # noqa: E402
from gan_amd.nets import Buf, Ctx  # noqa: E402
from gan_amd.steps import Pix2PixStep  # noqa: E402

POINTS = [(256, 16, 1), (256, 64, 1), (512, 8, 3)]      # size, batch, channels (section 12's table)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--step-batch', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dssim.py needs an MI355X"
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=64)
    lib = ctx.lib
    res = {'tool': 'bench_dssim', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'points': []}
    for S, B, ch in POINTS:
        pred, tar, grad = (Buf(ctx, B, S, S, 8) for _ in range(3))
        base = torch.rand(B, S, S, ch, device=ctx.device) * 2 - 1
        pred.t[..., :ch] = (0.8 * base + 0.2 * (torch.rand_like(base) * 2 - 1)).to(pred.t.dtype)
        tar.t[..., :ch] = base.to(tar.t.dtype)
        va, vb, vd = pred.view(0, ch), tar.view(0, ch), grad.view(0, ch)
        loss = torch.zeros(1, device=ctx.device)
        ws = torch.empty(max(lib.gan_dssim_workspace_bytes(B, S, S, ch), 4096 * 4) // 4, device=ctx.device)
        qws = torch.empty(lib.gan_image_quality_workspace_bytes(B, S, S, ch) // 4, device=ctx.device)
        rows = torch.empty(B, 4, device=ctx.device)

        def dssim(with_grad):
            d = L.GanDssimDesc(ctx.dt, ctx.dt, va, vb, 1.0, 0, loss.data_ptr(), 100.0, ctx.dt, vd if with_grad else L.GanTensor(),
                               ws.data_ptr(), ws.numel() * 4, None)
            return lambda: L.check(lib.gan_dssim(C.byref(d), ctx.stream()), 'dssim')
        l1 = lambda: L.check(lib.gan_l1(ctx.dt, C.byref(va), C.byref(vb), 1.0, 0, loss.data_ptr(), 100.0, C.byref(vd), ws.data_ptr(), None,
                                        ctx.stream()), 'l1')
        qd = L.GanQualityDesc(ctx.dt, ctx.dt, va, vb, rows.data_ptr(), qws.data_ptr(), qws.numel() * 4)
        quality = lambda: L.check(lib.gan_image_quality(C.byref(qd), ctx.stream()), 'image_quality')
        point = dict(size=S, batch=B, channels=ch, dtype='bf16', pitch=8)
        for name, fn in (('dssim_grad', dssim(True)), ('dssim_loss_only', dssim(False)), ('l1_grad', l1), ('image_quality', quality)):
            ms, n = timed(fn, a.min_seconds)
            point[name + '_us'] = 1e3 * ms
            point[name + '_calls'] = n
        res['points'].append(point)
        del pred, tar, grad

    # the captured training step, for information: same seeds and inputs, the secondary loss alone differs
    B = a.step_batch
    x, y = (torch.rand(B, 256, 256, 1, device=ctx.device) * 2 - 1 for _ in range(2))
    res['step'] = {'size': 256, 'batch': B, 'dtype': 'bf16'}
    for kind in ('l1', 'dssim', 'l1', 'dssim'):          # interleaved: two windows each
        st = Pix2PixStep(ctx, B, 256, 1, lam=100.0, seed=123, generator_loss=kind)
        replay = st.capture(training=True)
        ms, n = timed(lambda: replay(x, y), a.min_seconds)
        res['step'].setdefault(kind + '_ms', []).append(ms)
        res['step'].setdefault(kind + '_img_s', []).append(B * 1e3 / ms)
        del st, replay
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
