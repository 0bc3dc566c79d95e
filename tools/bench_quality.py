#!/usr/bin/env python3
"""Cost of the image-quality metrics: one `gan_image_quality` call beside one `gan_l1` launch on the same
operands, and one validation pass of tools/bench_epoch.py's synthetic set with `--quality-metrics` on and off.

    python tools/bench_quality.py [--min-seconds 1.0] [--n-val 256] [--out profiles/bench_quality.json]

Every point: warm-up, then HIP events around as many back-to-back calls as fill --min-seconds (tools/bench_infer.py's `timed`).
The validation pass is what `Pix2Pix.fit` adds per epoch with the flag on: the validation steps (captured step, training=False)
alone, against the same steps followed by the inference-mode evaluation of the same batches; wall time to the drain.  Prints one
JSON object; --out also saves it.  Reported, not gated."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch  # noqa: E402

from bench_epoch import write_pairs  # noqa: E402
from bench_infer import timed  # noqa: E402
from gan_amd import _lib as L  # noqa: E402
from gan_amd import data as D  # noqa: E402
from gan_amd import pix2pix  # noqa: E402
from gan_amd.nets import Buf, Ctx  # noqa: E402
from gan_amd.quality import QualityMeter, image_quality  # noqa: E402

POINTS = [(256, 16, 1, 'bf16'), (256, 64, 1, 'bf16'), (512, 8, 3, 'bf16')]      # size, batch, channels, prediction dtype (target fp32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--n-val', type=int, default=256, help='images of the synthetic validation set')
    ap.add_argument('--batch-size', type=int, default=16)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_quality.py needs an MI355X"
    ctx = Ctx('cuda:0', 'bf16', workspace_mb=64)
    lib = ctx.lib
    res = {'tool': 'bench_quality', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'points': []}
    for S, B, ch, dt in POINTS:
        pred = Buf(ctx, B, S, S, 8)                     # the generator's output layout: 8-channel-padded, typed
        pred.t[..., :ch] = (torch.rand(B, S, S, ch, device=ctx.device) * 2 - 1).to(pred.t.dtype)
        tar = torch.rand(B, S, S, ch, device=ctx.device) * 2 - 1
        out = torch.empty(B, 4, device=ctx.device)
        ms_q, n_q = timed(lambda: image_quality(ctx, pred, tar, out=out), a.min_seconds)
        # gan_l1 takes ONE dtype for both operands: the target packed to the prediction's layout, outside the timed region
        tar_t = Buf(ctx, B, S, S, 8)
        tar_t.t[..., :ch] = tar.to(tar_t.t.dtype)
        va, vb = pred.view(0, ch), tar_t.view(0, ch)
        loss, ws = torch.zeros(1, device=ctx.device), torch.empty(4096, device=ctx.device)
        l1 = lambda: L.check(lib.gan_l1(ctx.dt, C.byref(va), C.byref(vb), 1.0, 0, loss.data_ptr(), 0.0, None, ws.data_ptr(), None, ctx.stream()), 'l1')
        ms_l, n_l = timed(l1, a.min_seconds)
        bytes_read = B * S * S * ch * (pred.t.element_size() + 4)
        res['points'].append(dict(size=S, batch=B, channels=ch, pred_dtype=dt, target_dtype='f32', quality_us=1e3 * ms_q, quality_calls=n_q,
                                  quality_img_s=B * 1e3 / ms_q, real_bytes_read=bytes_read, l1_us=1e3 * ms_l, l1_calls=n_l,
                                  l1_note='both operands bf16 (gan_l1 has one dtype), same shapes and pitch'))
        del pred, tar, tar_t
    ctx = None
    torch.cuda.empty_cache()

    # one validation pass with the flag off / on
    with tempfile.TemporaryDirectory() as tmp:
        files = write_pairs(tmp, a.n_val, 256, 1, 123)
        opt = pix2pix.parse_opt(['--data', tmp, '--output', tmp, '--train', '--epochs', '1', '--batch-size', str(a.batch_size)])
        m = pix2pix.Pix2Pix(vars(opt))
        val = {'host': D.Batches(files, m.process_images_pred, a.batch_size, m.ctx.device),
               'device': D.DeviceBatches(D.DeviceDataset(files, 1, 256, m.ctx.device, 'pair', False, 'left'), a.batch_size,
                                         make_example=m.process_images_pred)}

        def val_pass(ds, quality):
            acc = None
            for x, y in ds:
                losses = torch.stack(m.train_step(x, y, False))
                acc = losses if acc is None else acc + losses
            acc.cpu()
            if quality:
                meter = QualityMeter()
                m._evaluate_into(meter, ds)
                meter.sums()[0].cpu()

        res['validation_pass'] = {'n_images': a.n_val, 'batch_size': a.batch_size, 'img_size': 256, 'dtype': 'bf16'}
        for name, ds in val.items():
            for quality in (False, True):
                val_pass(ds, quality)                   # warm-up (captures the step, builds the eval call)
                torch.cuda.synchronize()
                reps, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < a.min_seconds:
                    val_pass(ds, quality)
                    reps += 1
                torch.cuda.synchronize()
                dt_ = (time.perf_counter() - t0) / reps
                res['validation_pass'][f"{name}_cache_quality_{'on' if quality else 'off'}"] = {'seconds': dt_, 'passes': reps}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
