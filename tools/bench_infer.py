#!/usr/bin/env python3
"""Inference-mode generator throughput (`generator(x, training=False)`, BatchNorm folded into the convolutions) against the
batch-1 training-mode call that `--predict` makes by default (`generate_images`: `generator(x, training=True)`).

    python tools/bench_infer.py [--dtype bf16] [--size 256] [--batches 1,16,64] [--min-seconds 1.0]

Every point: warm-up, then HIP events around as many back-to-back calls as fill --min-seconds.  Prints one JSON object:
per batch the eval forward alone (folded weights current: fold=False), the call `--predict-training false` makes per batch
(pack + forward + unpack, folded once before), the full `model(x, training=False)` call (fold + pack + forward + unpack), the
fold launch alone, and the launch counts of one training-mode and one eval-mode forward (diag.launch_log)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gan_amd import _lib as L  # noqa: E402
from gan_amd.base_gan import GeneratorModel  # noqa: E402
from gan_amd.nets import Ctx, GeneratorNet  # noqa: E402


def timed(fn, min_s):
    """Mean milliseconds per call of fn() over >= min_s seconds, after warm-up (HIP events on the current stream)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 1e3 * min_s:
            return ms / n, n
        n = max(n * 2, int(n * 1.2e3 * min_s / max(ms, 1e-3)))


def launches(fn):
    torch.cuda.synchronize()
    L.set_option('diag.launch_log', 1)
    try:
        fn()
        torch.cuda.synchronize()
        return L.launch_log()
    finally:
        L.set_option('diag.launch_log', 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f16', 'f32'])
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--batches', default='1,16,64')
    ap.add_argument('--min-seconds', type=float, default=1.0)
    a = ap.parse_args()
    S = a.size
    ctx = Ctx('cuda:0', a.dtype)
    model = GeneratorModel(GeneratorNet(ctx, 1, 'batchnorm', seed=1))
    out = dict(metric='generator inference', dtype=a.dtype, size=S, min_seconds=a.min_seconds, device=torch.cuda.get_device_name(0))

    # reference point: the batch-1 training-mode call of --predict (pack, dropout masks, forward with batch statistics, unpack)
    x1 = torch.rand(1, S, S, 1, device=ctx.device) * 2 - 1
    ms, n = timed(lambda: model(x1, training=True), a.min_seconds)
    call = model._calls[(1, S)]
    out['train_mode_b1'] = dict(ms=ms, img_s=1e3 / ms, calls=n,
                                forward_launches=len(launches(lambda: (ctx.run(call.mask_ops), ctx.run(call.fwd_ops)))))
    model.fold()
    ms, n = timed(model.fold, a.min_seconds)
    out['fold'] = dict(ms=ms, calls=n, launches=len(launches(model.fold)))
    out['eval'] = {}
    for B in [int(b) for b in a.batches.split(',')]:
        x = torch.rand(B, S, S, 1, device=ctx.device) * 2 - 1
        model(x, training=False)                         # builds the call, folds
        ev = model._eval_calls[(B, S)]
        ms_fwd, n_fwd = timed(lambda: ev.infer(fold=False), a.min_seconds)
        ms_pred, n_pred = timed(lambda: model.infer(x, fold=False), a.min_seconds)     # what --predict-training false runs per batch
        ms_call, n_call = timed(lambda: model(x, training=False), a.min_seconds)
        out['eval'][str(B)] = dict(forward_ms=ms_fwd, forward_img_s=B * 1e3 / ms_fwd, forward_calls=n_fwd,
                                   predict_call_ms=ms_pred, predict_call_img_s=B * 1e3 / ms_pred, predict_call_calls=n_pred,
                                   call_ms=ms_call, call_img_s=B * 1e3 / ms_call, call_calls=n_call,
                                   forward_launches=len(launches(lambda: ev.infer(fold=False))),
                                   fold_and_forward_launches=len(launches(lambda: ev.infer(fold=True))))
        del ev
        model._eval_calls.clear()
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
