#!/usr/bin/env python3
"""Cost of the cycle-consistency metrics of a CycleGAN: what the glue around the forwards - the typed copy
between the two generators, gan_tile_gather, the metric launches, the torch slicing of the rows - adds to the forwards it wraps.

    python tools/bench_cycle_quality.py [--min-seconds 1.0] [--repeats 3] [--out profiles/bench_cycle_quality.json]

Two points, bf16, single channel, InstanceNorm generators:
  batch : cycle_quality(model, x) at 256 x 256, batch 16 - three eval forwards (G, then F twice: the cycle and the identity map)
          and two gan_image_quality calls.  (a) the three forwards alone on inputs already in the calls' buffers.
  tiled : cycle_quality_tiled on one 512 x 640 image, tiles of 256, overlap 64 (3 x 3 tiles per pass).  (a) two infer_tiled calls
          alone (G on the uint8 image, F on a float image).
  validation_pass : one validation pass of a --train run with --data-cache device (64 images per side, batch 16) without and with
          what --quality-metrics true adds to it; wall clock, host time included (validation_pass below).
Per point of the first two (a) and (b) alternate, HIP events around as many back-to-back calls as fill --min-seconds (tools/bench_infer.py's
`timed`), --repeats times each; the median is reported beside every repeat.  overhead = (b - a) / a.  Prints one JSON object;
--out also saves it.  Reported, not gated."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_infer import timed  # noqa: E402
from gan_amd import cycle_quality as Q  # noqa: E402
from gan_amd import tiling  # noqa: E402
from gan_amd.cycle_gan import CycleGAN  # noqa: E402

H, W, S, V, BATCH = 512, 640, 256, 64, 16


def validation_pass(repeats, n_val=64, batch=BATCH):
    """One validation pass of a --train run with --data-cache device, as runner.run_epochs makes it - the zipped validation sets
    through train_step(training=False), the losses drained once - and the same pass followed by what --quality-metrics true adds
    (CycleGAN._evaluate_into and the one drain of its sums).  Wall clock between device synchronisations, host time included: that
    is what a user waits for.  n_val synthetic 256 x 256 PNGs per side, decoded once before the clock starts."""
    import tempfile
    import time
    from PIL import Image
    from gan_amd.quality import QualityMeter
    rng = np.random.default_rng(1)
    with tempfile.TemporaryDirectory() as tmp:
        dirs = [os.path.join(tmp, d) for d in 'xy']
        n_files = int(n_val / 0.25) + 1                      # validation_size 0.25 of the files that are not test images
        for d in dirs:
            os.makedirs(d)
            for i in range(n_files):
                Image.fromarray(rng.integers(0, 256, (S, S), dtype=np.uint8), 'L').save(os.path.join(d, f"p{i}.png"))
        cfg = dict(img_size=S, channels='1', learning_rate=2e-4, beta_1=0.5, beta_2=0.999, seed=1, batch_size=batch, dtype='bf16',
                   input_images=dirs[0], target_images=dirs[1], test_img=1, validation_size=0.25, data_cache='device')
        cfg['lambda'] = 10
        model = CycleGAN(cfg)
        _, _, val_x, val_y, _ = model.image_pipeline(predict=False)

        def losses():
            acc = None
            for x, y in model._zipped(val_x, val_y):
                step = torch.stack(model.train_step(x, y, False))
                acc = step if acc is None else acc + step
            return acc.cpu()

        def with_metrics():
            losses()
            meter = QualityMeter()
            model._evaluate_into(meter, val_x, val_y)
            return meter.sums()[0].cpu()

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        losses(), with_metrics()                             # captures the step, builds the eval calls
        ta, tb = [], []
        for _ in range(max(repeats, 5)):
            ta.append(clock(losses))
            tb.append(clock(with_metrics))
        images = min(len(val_x.files), len(val_y.files))
    fa, fb = statistics.median(ta), statistics.median(tb)
    return dict(point='validation_pass', images_per_side=images, batch=batch, size=S, data_cache='device', clock='wall',
                losses_ms=fa, with_metrics_ms=fb, overhead=(fb - fa) / fa, losses_ms_repeats=ta, with_metrics_ms_repeats=tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--min-seconds', type=float, default=1.0)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_cycle_quality.py needs an MI355X"
    cfg = dict(img_size=S, channels='1', learning_rate=2e-4, beta_1=0.5, beta_2=0.999, seed=1, batch_size=BATCH, dtype='bf16')
    cfg['lambda'] = 10
    model = CycleGAN(cfg)
    G, F = model.generator_g, model.generator_f
    G.fold(), F.fold()
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.uniform(-1, 1, (BATCH, S, S, 1)).astype(np.float32)).to(model.ctx.device)
    src = torch.from_numpy(rng.integers(0, 256, (H, W, 1), dtype=np.uint8)).to(model.ctx.device)
    fake = tiling.infer_tiled(G, src, tile=S, overlap=V, fold=False)
    cg, cf = G.eval_call(BATCH, S), F.eval_call(BATCH, S)

    def forwards():
        cg.infer(fold=False)
        cf.infer(fold=False)
        cf.infer(fold=False)

    def two_tiled():
        tiling.infer_tiled(G, src, tile=S, overlap=V, fold=False)
        tiling.infer_tiled(F, fake, tile=S, overlap=V, fold=False)

    points = (('batch', forwards, lambda: Q.cycle_quality(model, x), dict(batch=BATCH, size=S)),
              ('tiled', two_tiled, lambda: Q.cycle_quality_tiled(model, src, tile=S, overlap=V), dict(image=[H, W, 1], tile=S, overlap=V)))
    res = {'tool': 'bench_cycle_quality', 'min_seconds': a.min_seconds, 'device': torch.cuda.get_device_name(0), 'dtype': 'bf16',
           'points': []}
    for name, alone, whole, what in points:
        whole()
        ta, tb = [], []
        for _ in range(a.repeats):
            ta.append(timed(alone, a.min_seconds)[0] * 1e3)
            tb.append(timed(whole, a.min_seconds)[0] * 1e3)
        fa, fb = statistics.median(ta), statistics.median(tb)
        res['points'].append(dict(point=name, **what, forwards_us=fa, with_metrics_us=fb, overhead=(fb - fa) / fa,
                                  forwards_us_repeats=ta, with_metrics_us_repeats=tb))
    res['points'].append(validation_pass(a.repeats))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
