#!/usr/bin/env python3
"""Cost of the MS-SSIM generator loss: one `gan_msssim` call (five scales) with its gradient, loss-only, and
with one scale and weight 1, beside one `gan_dssim` call and one `gan_l1` call (both with their gradients) on the same operands, at
the shapes of section 12's table; and the captured Pix2Pix training step at 256^2 bf16 with generator_loss 'l1', 'msssim' and
'msssim_l1' in interleaved windows (for information).

    python tools/bench_msssim.py [--min-seconds 1.0] [--step-batch 16] [--out profiles/bench_msssim.json]

Every point: the call alone as a captured graph, warm-up, then HIP events around as many back-to-back replays as fill --min-seconds
(tools/bench_infer.py's `timed`).  All operands in the step's layout: typed (bf16), 8-channel-padded buffers.  Prints one JSON
object; --out also saves it.  Reported, not gated."""
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
    assert torch.cuda.is_available(), "bench_msssim.py needs an MI355X"
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=64)
    lib = ctx.lib
    res = {'tool': 'bench_msssim', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'points': []}
    for S, B, ch in POINTS:
        pred, tar, grad = (Buf(ctx, B, S, S, 8) for _ in range(3))
        base = torch.rand(B, S, S, ch, device=ctx.device) * 2 - 1
        pred.t[..., :ch] = (0.8 * base + 0.2 * (torch.rand_like(base) * 2 - 1)).to(pred.t.dtype)
        tar.t[..., :ch] = base.to(tar.t.dtype)
        va, vb, vd = pred.view(0, ch), tar.view(0, ch), grad.view(0, ch)
        loss = torch.zeros(1, device=ctx.device)
        ws = torch.empty(max(lib.gan_msssim_workspace_bytes(B, S, S, ch, 5), 4096 * 4) // 4, device=ctx.device)

        def msssim(with_grad, scales):
            d = L.GanMsssimDesc(ctx.dt, ctx.dt, va, vb, 1.0, 0, loss.data_ptr(), 100.0, ctx.dt, vd if with_grad else L.GanTensor(),
                                ws.data_ptr(), ws.numel() * 4, None, scales, L.msssim_power(scales, (1.0,) if scales == 1 else None), None, 0)
            return lambda: L.check(lib.gan_msssim(C.byref(d), ctx.stream()), 'msssim')
        dd = L.GanDssimDesc(ctx.dt, ctx.dt, va, vb, 1.0, 0, loss.data_ptr(), 100.0, ctx.dt, vd, ws.data_ptr(), ws.numel() * 4, None)
        dssim = lambda: L.check(lib.gan_dssim(C.byref(dd), ctx.stream()), 'dssim')
        l1 = lambda: L.check(lib.gan_l1(ctx.dt, C.byref(va), C.byref(vb), 1.0, 0, loss.data_ptr(), 100.0, C.byref(vd), ws.data_ptr(), None,
                                        ctx.stream()), 'l1')
        point = dict(size=S, batch=B, channels=ch, dtype='bf16', pitch=8)
        for name, fn in (('msssim_grad', msssim(True, 5)), ('msssim_loss_only', msssim(False, 5)), ('msssim_one_scale_grad', msssim(True, 1)),
                         ('dssim_grad', dssim), ('l1_grad', l1)):
            torch.cuda.synchronize()
            graph = ctx.capture_graph(fn)
            ms, n = timed(graph.replay, a.min_seconds)
            point[name + '_us'] = 1e3 * ms
            point[name + '_calls'] = n
            del graph
        point['msssim_over_dssim'] = point['msssim_grad_us'] / point['dssim_grad_us']
        res['points'].append(point)
        del pred, tar, grad

    # the captured training step, for information: same seeds and inputs, the secondary loss alone differs
    B = a.step_batch
    x, y = (torch.rand(B, 256, 256, 1, device=ctx.device) * 2 - 1 for _ in range(2))
    res['step'] = {'size': 256, 'batch': B, 'dtype': 'bf16'}
    for kind in ('l1', 'msssim', 'msssim_l1') * 2:          # interleaved: two windows each
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
